"""Python face of the MI355X chunk-hash path (over liblbfhash.so).

Mirrors the reference's hash entry points so tests read like the reference's
own call sites:

* ``base64_encode(data)`` == ``libBitFlood::Encoder::Base64Encode``
  (/root/reference/cpp/src/Encoder.cpp:107-120): SHA-1 rendered as the
  27-char unpadded base64 string.
* ``ChunkHasher.hash_chunks`` == the per-chunk hash loop of
  ``Encoder::EncodeFile`` (Encoder.cpp:54-72), batched.
* ``ChunkHasher.verify_chunks`` == the compare-with-flood-file verify of
  ``Flood::_SetupFilesAndChunks`` (Flood.cpp:259-275) and of
  ``ChunkMethodHandler::_HandleSendChunk`` (ChunkMethods.cpp:165-167).
* ``ChunkHasher.update_chunks`` with ``new_states`` == the hash object
  underneath, fed piece by piece: Crypto++'s ``Update()`` ... ``Final()``
  (iterhash.cpp:9-99) as one resumable 96-byte state per chain.
* ``ChunkHasher.update_text`` with ``new_b64_states`` == xmlrpc++'s base64
  decoder (base64.h:215-330) in front of that object, fed the pieces of a
  SendChunk payload's text as they arrive (ChunkMethods.cpp:137-167): a
  16-byte decoder state beside each chain's hash state.
* ``ChunkHasher.update_encode`` with ``new_b64_enc_states`` == the seeder's
  re-verify and base64 encode (ChunkMethods.cpp:89-135, xmlrpc++'s encoder,
  base64.h:154-210) fed the pieces of a chunk as they are read: a 16-byte
  encoder state beside each chain's hash state, text in either peer layout.

All hashing runs on the GPU; there is no CPU path in this module.
"""
from __future__ import annotations

import ctypes
import os

import numpy as np

from . import _capi
from ._capi import LBF_DEVICE_PTR, LBF_HOST_PTR, LbfError, check, load

DIGEST = 20
# A valid one-byte host buffer that lives as long as the process: the base
# pointer for batches over empty data (every chunk then has size 0, so nothing
# is read from it, but the library still gets a real address).
_EMPTY = (ctypes.c_uint8 * 1)()


# lbf_sha1_state (lbf_hash.h): one resumable SHA-1 chain, 96 bytes.
STATE_DTYPE = np.dtype({"names": ["h", "buffered", "total", "block"],
                        "formats": [(np.uint32, 5), np.uint32, np.uint64, (np.uint8, 64)],
                        "offsets": [0, 20, 24, 32], "itemsize": 96})


def new_states(n: int) -> np.ndarray:
    """n fresh states, as lbf_sha1_state_init leaves them (host code, no GPU)."""
    states = np.zeros(int(n), dtype=STATE_DTYPE)
    if states.size:
        load().lbf_sha1_state_init(states.ctypes.data, states.size)
    return states


# lbf_b64_state (lbf_hash.h): xmlrpc++'s base64 decoder stopped between two
# pieces of a chunk's text, 16 bytes, the partner of the chain's STATE_DTYPE record.
B64_STATE_DTYPE = np.dtype({"names": ["decoded", "carry", "ncarry", "ended", "zero"],
                            "formats": [np.uint64, np.uint32, np.uint8, np.uint8, np.uint16],
                            "offsets": [0, 8, 12, 13, 14], "itemsize": 16})


def new_b64_states(n: int) -> np.ndarray:
    """n fresh decoder states, as lbf_b64_state_init leaves them (host code, no GPU)."""
    states = np.empty(int(n), dtype=B64_STATE_DTYPE)
    if states.size:
        load().lbf_b64_state_init(states.ctypes.data, states.size)
    return states


# lbf_b64_enc_state (lbf_hash.h): the base64 encoder stopped between two pieces
# of a chunk's bytes, 16 bytes, the partner of the chain's STATE_DTYPE record.
B64_ENC_STATE_DTYPE = np.dtype({"names": ["taken", "carry", "ncarry", "layout", "zero"],
                                "formats": [np.uint64, np.uint32, np.uint8, np.uint8, np.uint16],
                                "offsets": [0, 8, 12, 13, 14], "itemsize": 16})
B64_LAYOUTS = {"xmlrpc": 0, "flat": 1}  # LBF_B64_LAYOUT_*


def _layout(layout) -> int:
    if layout in B64_LAYOUTS:
        return B64_LAYOUTS[layout]
    if layout in (0, 1):
        return int(layout)
    raise ValueError("layout must be 'xmlrpc' or 'flat'")


def new_b64_enc_states(n: int, layout="xmlrpc") -> np.ndarray:
    """n fresh encoder states of one layout, as lbf_b64_enc_state_init leaves
    them (host code, no GPU)."""
    states = np.empty(int(n), dtype=B64_ENC_STATE_DTYPE)
    if states.size:
        load().lbf_b64_enc_state_init(states.ctypes.data, states.size, _layout(layout))
    return states


def b64_text_length(size: int, layout="xmlrpc") -> int:
    """lbf_b64_text_length: characters of the whole text of a chunk of `size` bytes."""
    return int(load().lbf_b64_text_length(int(size), _layout(layout)))


def b64_27(digest: bytes) -> str:
    """20-byte digest -> 27-char string (basecode.cpp:39-104, no padding)."""
    if len(digest) != DIGEST:
        raise ValueError("digest must be 20 bytes")
    out = ctypes.create_string_buffer(28)
    load().lbf_b64_27(bytes(digest), out)
    return out.value.decode()


def b64_27_decode(s: str) -> bytes:
    raw = s.encode()
    out = (ctypes.c_uint8 * DIGEST)()
    check(load().lbf_b64_27_decode(raw, len(raw), out))
    return bytes(out)


def chunk_table(length: int, chunk_size: int, base_offset: int = 0):
    """Offsets/sizes of Encoder.cpp's fixed-size chunking of one file:
    chunk i = [i*cs, min((i+1)*cs, length)); an empty file has no chunks."""
    if chunk_size <= 0:
        raise ValueError("chunk_size must be positive")
    n = (length + chunk_size - 1) // chunk_size
    offs = np.arange(n, dtype=np.uint64) * np.uint64(chunk_size)
    sizes = np.full(n, chunk_size, dtype=np.uint32)
    if n:
        sizes[-1] = length - (n - 1) * chunk_size
    return offs + np.uint64(base_offset), sizes


def chain_table(state_of):
    """The chain table the *_seq_launch calls read, from the state each piece
    names: (order, chain_state, chain_first).  A stable grouping: chains stand
    in the order their first pieces stand in `state_of`, and a chain's pieces
    keep their order.  order[j] is the caller's piece at table position j (lay
    the per-piece arrays out as arr[order]; results at position j belong to
    piece order[j]), chain c continues state chain_state[c], and its pieces are
    table positions [chain_first[c], chain_first[c + 1]).  When no state repeats
    order is the identity and chain_state equals state_of."""
    so = np.ascontiguousarray(state_of, dtype=np.uint32).reshape(-1)
    if so.size == 0:
        return np.zeros(0, dtype=np.uint32), np.zeros(0, dtype=np.uint32), np.zeros(1, dtype=np.uint32)
    states, first_at, chain_of = np.unique(so, return_index=True, return_inverse=True)
    by_first = np.argsort(first_at, kind="stable")  # chains in the order of their first pieces
    rank = np.empty(by_first.size, dtype=np.int64)
    rank[by_first] = np.arange(by_first.size)
    chain = rank[chain_of.reshape(-1)]
    order = np.argsort(chain, kind="stable").astype(np.uint32)
    chain_first = np.zeros(by_first.size + 1, dtype=np.uint32)
    chain_first[1:] = np.cumsum(np.bincount(chain, minlength=by_first.size))
    return order, states[by_first].astype(np.uint32), chain_first


def _as_u8(data) -> np.ndarray:
    if isinstance(data, np.ndarray):
        return np.ascontiguousarray(data).view(np.uint8).reshape(-1)
    return np.frombuffer(memoryview(data), dtype=np.uint8)


class ChunkHasher:
    """An lbf_ctx: device buffers, streams and pinned staging on one or more GPUs."""

    def __init__(self, device_mask: int = 0):
        lib = load()
        h = ctypes.c_void_p()
        check(lib.lbf_ctx_create(device_mask, ctypes.byref(h)))
        self._h = h
        self._lib = lib
        self._registered = {}  # pointer -> array kept alive while pinned

    @property
    def num_devices(self) -> int:
        return self._lib.lbf_ctx_num_devices(self._h)

    @property
    def num_workers(self) -> int:
        return self._lib.lbf_ctx_num_workers(self._h)

    def worker_info(self, worker: int = 0) -> dict:
        """Device, its NUMA node, the node of the worker's pinned staging and the
        number of CPUs its host threads are bound to (see lbf_ctx_worker_info)."""
        v = [ctypes.c_int(-9) for _ in range(4)]
        check(self._lib.lbf_ctx_worker_info(self._h, worker, *[ctypes.byref(x) for x in v]))
        return dict(zip(["device", "numa_node", "staging_node", "bound_cpus"], [x.value for x in v]))

    def close(self) -> None:
        if self._h:
            self._lib.lbf_ctx_destroy(self._h)
            self._h = None
        self._registered = {}

    def staging_stats(self) -> dict:
        """Cumulative chunk bytes sent through pinned staging / straight from
        registered memory (lbf_ctx_staging_stats)."""
        st, di = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._lib.lbf_ctx_staging_stats(self._h, ctypes.byref(st), ctypes.byref(di)))
        return {"staged": st.value, "direct": di.value}

    def b64_stats(self) -> dict:
        """Chunks of verify_b64 calls so far by decode path: text with the
        encoder's own layout decoded in one pass, the rest by the general
        two-pass kernel (lbf_ctx_b64_stats)."""
        one, gen = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._lib.lbf_ctx_b64_stats(self._h, ctypes.byref(one), ctypes.byref(gen)))
        return {"one_pass": one.value, "general": gen.value}

    def b64_update_stats(self) -> dict:
        """Characters of update_text calls so far by decode path: the prefixes
        that continued the encoder's layout and went through line tiles, and the
        rest, decoded by the general rule (lbf_ctx_b64_update_stats)."""
        line, scan = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._lib.lbf_ctx_b64_update_stats(self._h, ctypes.byref(line), ctypes.byref(scan)))
        return {"line_chars": line.value, "scan_chars": scan.value}

    def b64_flat_stats(self) -> dict:
        """The flat path's share of the two counters above: verify_b64's chunks
        of unbroken text that the flat pass decoded (counted in "general" too)
        and update_text's characters that the flat kernel took (counted in
        "scan_chars" too) (lbf_ctx_b64_flat_stats)."""
        chunks, chars = ctypes.c_uint64(0), ctypes.c_uint64(0)
        check(self._lib.lbf_ctx_b64_flat_stats(self._h, ctypes.byref(chunks), ctypes.byref(chars)))
        return {"flat_chunks": chunks.value, "flat_chars": chars.value}

    # -- caller-pinned sources (lbf_host_register) ---------------------------
    def register_host(self, data) -> None:
        """Pin `data` (a contiguous numpy array / buffer) for this context:
        batches over it then go to the GPU without the staging copy.  The array
        is kept alive until unregister_host / close."""
        if isinstance(data, np.ndarray) and not data.flags.c_contiguous:
            raise ValueError("register_host: the array must be C-contiguous (a copy would be pinned instead)")
        buf = _as_u8(data)
        if buf.size == 0:
            raise ValueError("register_host: empty buffer")
        check(self._lib.lbf_host_register(self._h, buf.ctypes.data, buf.size))
        self._registered[buf.ctypes.data] = buf

    def unregister_host(self, data) -> None:
        ptr = _as_u8(data).ctypes.data
        check(self._lib.lbf_host_unregister(self._h, ptr))
        self._registered.pop(ptr, None)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- host-memory batches -------------------------------------------------
    def hash_chunks(self, data, offsets, sizes) -> np.ndarray:
        buf = _as_u8(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        if offs.shape != szs.shape:
            raise ValueError("offsets and sizes differ in length")
        n = offs.size
        out = np.zeros((n, DIGEST), dtype=np.uint8)
        if n == 0:
            return out
        base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
        check(self._lib.lbf_sha1_batch(self._h, base, buf.size, offs.ctypes.data, szs.ctypes.data, n,
                                       out.ctypes.data, LBF_HOST_PTR))
        return out

    def verify_chunks(self, data, offsets, sizes, expected) -> np.ndarray:
        buf = _as_u8(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        n = offs.size
        if szs.size != n or exp.shape[0] != n:
            raise ValueError("offsets, sizes and expected differ in length")
        ver = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return ver.astype(bool)
        base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
        check(self._lib.lbf_verify_batch(self._h, base, buf.size, offs.ctypes.data, szs.ctypes.data, n,
                                         exp.ctypes.data, ver.ctypes.data, LBF_HOST_PTR))
        return ver.astype(bool)

    # -- chunks hashed piece by piece (lbf_sha1_update_batch) -------------------
    def update_chunks(self, states, data, offsets, sizes, state_of=None, final=None, expected=None) -> np.ndarray:
        """Absorb piece i = data[offsets[i], + sizes[i]) into states[state_of[i]]
        (states[i] without state_of); `states` (from new_states, or restored
        from bytes) is updated in place.  A piece with final[i] set ends its
        chain, as Crypto++'s Final() does (iterhash.cpp:86-99): its digest is
        row i of the (n, 20) result and its state is fresh again; rows of the
        other pieces are zero.  With `expected` the result is the bool verdicts
        instead (False for pieces that are not final)."""
        return self._update_chunks(self._lib.lbf_sha1_update_batch, states, data, offsets, sizes, state_of, final,
                                   expected)

    def update_chunks_seq(self, states, data, offsets, sizes, state_of=None, final=None, expected=None) -> np.ndarray:
        """update_chunks without "at most one piece per state" (lbf_sha1_update_seq_batch):
        pieces that name one state are absorbed in the order they stand in the
        call, each touched state travels once per launch, and the results are
        at the caller's piece indices.  A final piece must be the last piece of
        its state in the call.  A call in which no state repeats returns what
        update_chunks returns."""
        return self._update_chunks(self._lib.lbf_sha1_update_seq_batch, states, data, offsets, sizes, state_of, final,
                                   expected)

    def _update_chunks(self, call, states, data, offsets, sizes, state_of, final, expected) -> np.ndarray:
        if not (isinstance(states, np.ndarray) and states.dtype == STATE_DTYPE and states.ndim == 1
                and states.flags.c_contiguous and states.flags.writeable):
            raise ValueError("states must be a writable C-contiguous 1-d array of STATE_DTYPE")
        buf = _as_u8(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        n = offs.size
        if szs.size != n:
            raise ValueError("offsets and sizes differ in length")
        so = None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32)
        fin = None if final is None else np.ascontiguousarray(final).astype(bool).astype(np.uint8)
        exp = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        for a, what in ((so, "state_of"), (fin, "final"), (exp, "expected")):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"{what} differs in length")
        out = np.zeros((n, DIGEST), dtype=np.uint8)
        ver = np.zeros(n, dtype=np.uint8)
        if n:
            base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
            ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            check(call(self._h, states.ctypes.data, states.size, ptr(so), base, buf.size, offs.ctypes.data,
                       szs.ctypes.data, ptr(fin), n, None if exp is not None else out.ctypes.data, ptr(exp),
                       None if exp is None else ver.ctypes.data))
        return out if exp is None else ver.astype(bool)

    # -- chunks' base64 text decoded and hashed piece by piece (lbf_b64_update_batch)
    def update_text(self, b64_states, sha_states, text, text_offsets, text_lens, out, out_offsets, expected_sizes,
                    state_of=None, final=None, expected=None):
        """Piece i = the base64 text text[text_offsets[i], + text_lens[i]) continues
        chain state_of[i] (chain i without state_of): the pair b64_states[s],
        sha_states[s] (from new_b64_states / new_states, or restored from bytes),
        updated in place.  Its chunk is expected_sizes[i] bytes at
        out[out_offsets[i] ..); the bytes the piece decodes land there at their
        place in the chunk, and no other byte of `out` is written.  A piece with
        final[i] set ends its chain.  Returns (out_sizes, verdicts): for a final
        piece the decoded length (expected_sizes[i] + 1 when more) and, with
        `expected`, whether length and SHA-1 are the chunk's; entries of the other
        pieces are 0 / False."""
        return self._update_text(self._lib.lbf_b64_update_batch, b64_states, sha_states, text, text_offsets,
                                 text_lens, out, out_offsets, expected_sizes, state_of, final, expected)

    def update_text_seq(self, b64_states, sha_states, text, text_offsets, text_lens, out, out_offsets, expected_sizes,
                        state_of=None, final=None, expected=None):
        """update_text without "at most one piece per state" (lbf_b64_update_seq_batch):
        pieces that name one chain -- the frames of one chunk a receiver holds
        when it drains its sockets -- are decoded and absorbed in the order they
        stand in the call; they repeat the chain's slot and chunk size.  A final
        piece must be the last piece of its chain in the call.  A call in which
        no chain repeats returns what update_text returns."""
        return self._update_text(self._lib.lbf_b64_update_seq_batch, b64_states, sha_states, text, text_offsets,
                                 text_lens, out, out_offsets, expected_sizes, state_of, final, expected)

    def _update_text(self, call, b64_states, sha_states, text, text_offsets, text_lens, out, out_offsets,
                     expected_sizes, state_of, final, expected):
        for st, dt, what in ((b64_states, B64_STATE_DTYPE, "b64_states"), (sha_states, STATE_DTYPE, "sha_states")):
            if not (isinstance(st, np.ndarray) and st.dtype == dt and st.ndim == 1 and st.flags.c_contiguous
                    and st.flags.writeable):
                raise ValueError(f"{what} must be a writable C-contiguous 1-d array of its state dtype")
        if b64_states.size != sha_states.size:
            raise ValueError("b64_states and sha_states differ in length")
        if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous
                and out.flags.writeable):
            raise ValueError("out must be a writable C-contiguous uint8 array")
        buf = _as_u8(text)
        toff = np.ascontiguousarray(text_offsets, dtype=np.uint64)
        tlen = np.ascontiguousarray(text_lens, dtype=np.uint32)
        ooff = np.ascontiguousarray(out_offsets, dtype=np.uint64)
        esz = np.ascontiguousarray(expected_sizes, dtype=np.uint32)
        n = toff.size
        if not (tlen.size == ooff.size == esz.size == n):
            raise ValueError("text_offsets, text_lens, out_offsets and expected_sizes differ in length")
        so = None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32)
        fin = None if final is None else np.ascontiguousarray(final).astype(bool).astype(np.uint8)
        exp = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        for a, what in ((so, "state_of"), (fin, "final"), (exp, "expected")):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"{what} differs in length")
        sizes = np.zeros(n, dtype=np.uint32)
        ver = np.zeros(n, dtype=np.uint8)
        if n:
            base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
            ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            check(call(self._h, b64_states.ctypes.data, sha_states.ctypes.data, b64_states.size, ptr(so), base,
                       buf.size, toff.ctypes.data, tlen.ctypes.data, ptr(fin), n, esz.ctypes.data, ptr(exp),
                       out.ctypes.data if out.size else None, out.size, ooff.ctypes.data, sizes.ctypes.data,
                       None if exp is None else ver.ctypes.data))
        return sizes, ver.astype(bool)

    # -- chunks to send, encoded and hashed piece by piece (lbf_b64_encode_update_batch)
    def update_encode(self, enc_states, states, data, offsets, sizes, text, text_offsets, text_caps, state_of=None,
                      final=None, expected=None):
        """Piece i = data[offsets[i], + sizes[i]) continues chain state_of[i] (chain
        i without state_of): the pair enc_states[s], states[s] (from
        new_b64_enc_states / new_states, or restored from bytes), updated in place.
        Its chunk's text slot is text[text_offsets[i], + text_caps[i]) (`text` a
        writable uint8 array); the characters the piece produces land there at
        their place in the chunk's text, and no other byte of `text` is written.
        Returns (new_offsets, new_lens): where in `text` each piece's new
        characters lie and how many there are.  With `final`, a piece with
        final[i] set ends its chain, and the result is (new_offsets, new_lens,
        text_sizes, verdicts): for a final piece the chunk's text length
        (text_caps[i] + 1 when it does not fit) and, with `expected`, whether the
        text fits and the SHA-1 is the chunk's; entries of the other pieces are
        0 / False."""
        for st, dt, what in ((enc_states, B64_ENC_STATE_DTYPE, "enc_states"), (states, STATE_DTYPE, "states")):
            if not (isinstance(st, np.ndarray) and st.dtype == dt and st.ndim == 1 and st.flags.c_contiguous
                    and st.flags.writeable):
                raise ValueError(f"{what} must be a writable C-contiguous 1-d array of its state dtype")
        if enc_states.size != states.size:
            raise ValueError("enc_states and states differ in length")
        if not (isinstance(text, np.ndarray) and text.dtype == np.uint8 and text.flags.c_contiguous
                and text.flags.writeable):
            raise ValueError("text must be a writable C-contiguous uint8 array")
        buf = _as_u8(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        toff = np.ascontiguousarray(text_offsets, dtype=np.uint64)
        caps = np.ascontiguousarray(text_caps, dtype=np.uint32)
        n = offs.size
        if not (szs.size == toff.size == caps.size == n):
            raise ValueError("offsets, sizes, text_offsets and text_caps differ in length")
        so = None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32)
        fin = None if final is None else np.ascontiguousarray(final).astype(bool).astype(np.uint8)
        exp = None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        for a, what in ((so, "state_of"), (fin, "final"), (exp, "expected")):
            if a is not None and a.shape[0] != n:
                raise ValueError(f"{what} differs in length")
        new_off = np.zeros(n, dtype=np.uint64)
        new_len = np.zeros(n, dtype=np.uint32)
        tsizes = np.zeros(n, dtype=np.uint32)
        ver = np.zeros(n, dtype=np.uint8)
        if n:
            base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
            ptr = lambda a: None if a is None else a.ctypes.data  # noqa: E731
            check(self._lib.lbf_b64_encode_update_batch(self._h, enc_states.ctypes.data, states.ctypes.data,
                                                        enc_states.size, ptr(so), base, buf.size, offs.ctypes.data,
                                                        szs.ctypes.data, ptr(fin), n, ptr(exp),
                                                        None if exp is None else ver.ctypes.data,
                                                        text.ctypes.data if text.size else None, text.size,
                                                        toff.ctypes.data, caps.ctypes.data, new_off.ctypes.data,
                                                        new_len.ctypes.data, tsizes.ctypes.data))
        if final is None:
            return new_off, new_len
        return new_off, new_len, tsizes, ver.astype(bool)

    # -- chunks read straight from a file (lbf_file_ranges) ---------------------
    def hash_file(self, path: str, offsets, sizes) -> np.ndarray:
        """Digests of byte ranges of a file, pread into pinned staging: EncodeFile's
        fread -> Base64Encode loop (Encoder.cpp:54-72) as one call."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        if offs.shape != szs.shape:
            raise ValueError("offsets and sizes differ in length")
        out = np.zeros((offs.size, DIGEST), dtype=np.uint8)
        if offs.size:
            check(self._lib.lbf_file_ranges(self._h, os.fsencode(path), offs.ctypes.data, szs.ctypes.data,
                                            offs.size, None, out.ctypes.data))
        return out

    def verify_file(self, path: str, offsets, sizes, expected) -> np.ndarray:
        """Resume verify of a file (Flood.cpp:259-275): True where the chunk is present
        in full and matches; short or missing chunks are False, as the reference leaves
        them '0'."""
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        if szs.size != offs.size or exp.shape[0] != offs.size:
            raise ValueError("offsets, sizes and expected differ in length")
        ver = np.zeros(offs.size, dtype=np.uint8)
        if offs.size:
            check(self._lib.lbf_file_ranges(self._h, os.fsencode(path), offs.ctypes.data, szs.ctypes.data,
                                            offs.size, exp.ctypes.data, ver.ctypes.data))
        return ver.astype(bool)

    def _files_call(self, paths, file_of, offsets, sizes, expected):
        enc = [os.fsencode(p) for p in paths]
        arr = (ctypes.c_char_p * len(enc))(*enc)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        szs = np.ascontiguousarray(sizes, dtype=np.uint32)
        fo = np.ascontiguousarray(file_of, dtype=np.uint32)
        if not (offs.shape == szs.shape == fo.shape):
            raise ValueError("file_of, offsets and sizes differ in length")
        if expected is None:
            out = np.zeros((offs.size, DIGEST), dtype=np.uint8)
            exp_ptr = None
        else:
            exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
            if exp.shape[0] != offs.size:
                raise ValueError("expected differs in length")
            out = np.zeros(offs.size, dtype=np.uint8)
            exp_ptr = exp.ctypes.data
        if offs.size:
            check(self._lib.lbf_files_ranges(self._h, arr, len(enc), fo.ctypes.data, offs.ctypes.data,
                                             szs.ctypes.data, offs.size, exp_ptr, out.ctypes.data))
        return out

    def hash_files(self, paths, file_of, offsets, sizes) -> np.ndarray:
        """Digests of byte ranges of several files in one pipelined batch
        (lbf_files_ranges): chunk i = [offsets[i], +sizes[i]) of paths[file_of[i]]."""
        return self._files_call(paths, file_of, offsets, sizes, None)

    def verify_files(self, paths, file_of, offsets, sizes, expected) -> np.ndarray:
        """Resume verify over several files in one batch (Flood.cpp:239-287)."""
        return self._files_call(paths, file_of, offsets, sizes, expected).astype(bool)

    def verify_b64(self, text, text_offsets, text_lens, expected_sizes, expected, out=None, out_offsets=None):
        """The receiver's decode + verify on the device (lbf_b64_verify_batch,
        ChunkMethods.cpp:137-167 with xmlrpc++'s base64 decode): chunk i is
        the base64 text text[text_offsets[i], + text_lens[i]).  Returns
        (verdicts as bool, decoded lengths); with `out` (a uint8 array) and
        `out_offsets` the decoded bytes land at out[out_offsets[i], +
        expected_sizes[i])."""
        buf = _as_u8(text)
        toff = np.ascontiguousarray(text_offsets, dtype=np.uint64)
        tlen = np.ascontiguousarray(text_lens, dtype=np.uint32)
        esz = np.ascontiguousarray(expected_sizes, dtype=np.uint32)
        exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        n = toff.size
        if not (tlen.size == esz.size == exp.shape[0] == n):
            raise ValueError("text_offsets, text_lens, expected_sizes and expected differ in length")
        ver = np.zeros(n, dtype=np.uint8)
        sizes = np.zeros(n, dtype=np.uint32)
        if n == 0:
            return ver.astype(bool), sizes
        ooff = None
        if out is not None:
            if not (isinstance(out, np.ndarray) and out.dtype == np.uint8 and out.flags.c_contiguous):
                raise ValueError("out must be a C-contiguous uint8 array")
            ooff = np.ascontiguousarray(out_offsets, dtype=np.uint64)
            if ooff.size != n:
                raise ValueError("out_offsets differs in length")
        base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
        check(self._lib.lbf_b64_verify_batch(self._h, base, buf.size, toff.ctypes.data, tlen.ctypes.data, n,
                                             esz.ctypes.data, exp.ctypes.data,
                                             None if out is None else out.ctypes.data,
                                             0 if out is None else out.size,
                                             None if ooff is None else ooff.ctypes.data, sizes.ctypes.data,
                                             ver.ctypes.data))
        return ver.astype(bool), sizes

    def verify_encode_b64(self, data, offsets, sizes, expected, layout="xmlrpc"):
        """The sender's verify + encode on the device
        (lbf_verify_encode_b64_layout_batch, ChunkMethods.cpp:89-135 with the
        base64 encode of `layout`: "xmlrpc", xmlrpc++'s lines, or "flat", the
        unbroken text of the Java and Perl peers): chunk i = data[offsets[i], +
        sizes[i]).  Returns (verdicts as bool, [text of chunk i as bytes])."""
        lay = _layout(layout)
        buf = _as_u8(data)
        offs = np.ascontiguousarray(offsets, dtype=np.uint64)
        sz = np.ascontiguousarray(sizes, dtype=np.uint32)
        exp = np.ascontiguousarray(expected, dtype=np.uint8).reshape(-1, DIGEST)
        n = offs.size
        if not (sz.size == exp.shape[0] == n):
            raise ValueError("offsets, sizes and expected differ in length")
        ver = np.zeros(n, dtype=np.uint8)
        if n == 0:
            return ver.astype(bool), []
        lens = [int(self._lib.lbf_b64_text_length(int(s), lay)) for s in sz]
        toff = np.zeros(n, dtype=np.uint64)
        pos = 0
        for i, tl in enumerate(lens):
            toff[i] = pos
            pos += (tl + 15) // 16 * 16
        text = np.zeros(max(pos, 1), dtype=np.uint8)
        base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
        check(self._lib.lbf_verify_encode_b64_layout_batch(self._h, base, buf.size, offs.ctypes.data, sz.ctypes.data,
                                                           n, exp.ctypes.data, ver.ctypes.data, lay, text.ctypes.data,
                                                           text.size, toff.ctypes.data))
        return ver.astype(bool), [text[int(toff[i]):int(toff[i]) + lens[i]].tobytes() for i in range(n)]

    def sha1(self, data) -> bytes:
        buf = _as_u8(data)
        out = (ctypes.c_uint8 * DIGEST)()
        base = buf.ctypes.data if buf.size else ctypes.addressof(_EMPTY)
        check(self._lib.lbf_sha1_one(self._h, base, buf.size, out))
        return bytes(out)

    def base64_encode(self, data) -> str:
        """Encoder::Base64Encode(data, size, out) (Encoder.cpp:107-120)."""
        return b64_27(self.sha1(data))

    def encode_buffer(self, data, chunk_size: int) -> list[str]:
        """Per-chunk hash strings of one in-memory file (Encoder.cpp:54-72)."""
        buf = _as_u8(data)
        offs, sizes = chunk_table(buf.size, chunk_size)
        return [b64_27(bytes(d)) for d in self.hash_chunks(buf, offs, sizes)]


# ---------------------------------------------------------------------------
# Device-resident helpers (bench.py, parity tests at full size)
# ---------------------------------------------------------------------------
class DeviceBuffer:
    def __init__(self, nbytes: int):
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(load().lbf_dev_malloc(ctypes.byref(p), self.nbytes))
        self.ptr = p.value

    def free(self):
        if self.ptr:
            check(load().lbf_dev_free(self.ptr))
            self.ptr = None

    def _range(self, offset: int, nbytes: int, what: str):
        if not self.ptr:
            raise ValueError(f"{what}: buffer already freed")
        if offset < 0 or nbytes < 0 or offset + nbytes > self.nbytes:
            raise ValueError(f"{what}: [{offset}, {offset + nbytes}) outside the {self.nbytes}-byte buffer")

    def upload(self, host: np.ndarray, offset: int = 0):
        host = np.ascontiguousarray(host)
        self._range(offset, host.nbytes, "upload")
        check(load().lbf_memcpy_h2d(self.ptr + offset, host.ctypes.data, host.nbytes))

    def download(self, nbytes: int | None = None, offset: int = 0, dtype=np.uint8) -> np.ndarray:
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        self._range(offset, nbytes, "download")
        out = np.empty(nbytes, dtype=np.uint8)
        check(load().lbf_memcpy_d2h(out.ctypes.data, self.ptr + offset, nbytes))
        return out.view(dtype)

    def download_into(self, out: np.ndarray, offset: int = 0) -> None:
        """Copy out.nbytes bytes from this buffer at `offset` into the existing
        C-contiguous host array `out`."""
        if not isinstance(out, np.ndarray) or not out.flags.c_contiguous:
            raise ValueError("download_into: out must be a C-contiguous numpy array")
        self._range(offset, out.nbytes, "download_into")
        if out.nbytes:
            check(load().lbf_memcpy_d2h(out.ctypes.data, self.ptr + offset, out.nbytes))

    def fill_synthetic(self, seed: int, start: int = 0, nbytes: int | None = None, stream=None, offset: int = 0):
        """Bytes [start, start+nbytes) of synthetic stream `seed` into this
        buffer at byte `offset` (16-byte aligned)."""
        nbytes = self.nbytes - offset if nbytes is None else nbytes
        self._range(offset, nbytes, "fill_synthetic")
        check(load().lbf_fill_synthetic(self.ptr + offset, nbytes, seed, start, stream))


def uniform_launch(base: DeviceBuffer | int, length: int, chunk_size: int, first: int, n: int,
                   digests: DeviceBuffer | int | None, expected=None, verdicts=None, stream=None):
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_sha1_uniform_launch(p(base), length, chunk_size, first, n, p(digests), p(expected),
                                         p(verdicts), stream))


def batch_launch(base, offsets, sizes, n, digests, expected=None, verdicts=None, stream=None):
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_sha1_launch(p(base), p(offsets), p(sizes), n, p(digests), p(expected), p(verdicts),
                                 stream))


def update_launch(states, n_states, state_of, base, offsets, sizes, final, n, digests, expected=None, verdicts=None,
                  stream=None):
    """lbf_sha1_update_launch: pieces in device memory absorbed into device-resident
    states, asynchronous on `stream`; state_of, final and the outputs may be None."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_sha1_update_launch(p(states), n_states, p(state_of), p(base), p(offsets), p(sizes), p(final), n,
                                        p(digests), p(expected), p(verdicts), stream))


def update_seq_launch(states, n_states, chain_state, chain_first, n_chains, base, offsets, sizes, final, n, digests,
                      expected=None, verdicts=None, stream=None):
    """lbf_sha1_update_seq_launch: update_launch with several pieces per chain,
    absorbed in table order; chain_state / chain_first are the chain table
    (chain_table), chain_state may be None (chain c continues state c)."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_sha1_update_seq_launch(p(states), n_states, p(chain_state), p(chain_first), n_chains, p(base),
                                            p(offsets), p(sizes), p(final), n, p(digests), p(expected), p(verdicts),
                                            stream))


def b64_update_seq_launch(b64_states, sha_states, n_states, chain_state, chain_first, n_chains, text, text_offsets,
                          text_lens, final, n, out, out_offsets, caps, out_sizes, digests, expected, verdicts,
                          piece_offsets, piece_sizes, stream=None):
    """lbf_b64_update_seq_launch: b64_update_launch with several pieces per chain,
    decoded and absorbed in table order, in three enqueues whatever their number."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_b64_update_seq_launch(p(b64_states), p(sha_states), n_states, p(chain_state), p(chain_first),
                                           n_chains, p(text), p(text_offsets), p(text_lens), p(final), n, p(out),
                                           p(out_offsets), p(caps), p(out_sizes), p(digests), p(expected), p(verdicts),
                                           p(piece_offsets), p(piece_sizes), stream))


def b64_update_launch(b64_states, sha_states, n_states, state_of, text, text_offsets, text_lens, final, n, out,
                      out_offsets, caps, out_sizes, digests, expected, verdicts, piece_offsets, piece_sizes,
                      stream=None):
    """lbf_b64_update_launch: pieces of text in device memory decoded into their
    chunks' slots and absorbed into device-resident state pairs, asynchronous on
    `stream`; state_of, final, digests and expected/verdicts may be None."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_b64_update_launch(p(b64_states), p(sha_states), n_states, p(state_of), p(text), p(text_offsets),
                                       p(text_lens), p(final), n, p(out), p(out_offsets), p(caps), p(out_sizes),
                                       p(digests), p(expected), p(verdicts), p(piece_offsets), p(piece_sizes), stream))


def b64_encode_update_launch(enc_states, sha_states, n_states, state_of, base, offsets, sizes, final, n, text,
                             text_offsets, text_caps, new_offsets, new_lens, text_sizes, digests, expected, verdicts,
                             stream=None):
    """lbf_b64_encode_update_launch: pieces of bytes in device memory encoded into
    their chunks' text slots and absorbed into device-resident state pairs,
    asynchronous on `stream`; state_of, final, digests and expected/verdicts may
    be None."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_b64_encode_update_launch(p(enc_states), p(sha_states), n_states, p(state_of), p(base),
                                              p(offsets), p(sizes), p(final), n, p(text), p(text_offsets),
                                              p(text_caps), p(new_offsets), p(new_lens), p(text_sizes), p(digests),
                                              p(expected), p(verdicts), stream))


def verify_encode_b64_launch(base, offsets, sizes, n, max_size, text, text_offsets, layout="xmlrpc", digests=None,
                             expected=None, verdicts=None, stream=None):
    """lbf_verify_encode_b64_launch: chunks in device memory hashed (digests
    and/or expected + verdicts; with none of them the call only encodes) and
    encoded into their text slots in one layout, asynchronous on `stream`;
    max_size is the largest chunk and sizes the grids."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_verify_encode_b64_launch(p(base), p(offsets), p(sizes), n, max_size, p(digests), p(expected),
                                              p(verdicts), _layout(layout), p(text), p(text_offsets), stream))


def b64_verify_launch_work(n: int) -> int:
    """lbf_b64_verify_launch_work: the bytes of `work` verify_b64_launch needs for n chunks."""
    return int(load().lbf_b64_verify_launch_work(n))


def verify_b64_launch(text, text_offsets, text_lens, n, max_text_len, expected_sizes, max_size, out, out_offsets,
                      out_sizes, work, digests=None, expected=None, verdicts=None, stream=None):
    """lbf_b64_verify_launch: chunk text in device memory (either peer layout, or
    anything else, mixed in one call) decoded into its slots and verified,
    asynchronous on `stream`; max_text_len and max_size are the longest text and
    the largest expected size and size the grids.  `work` is
    b64_verify_launch_work(n) bytes: behind the call work[0, n) is `over` and
    work[n, 2n) is `redo` (1 = the chunk went to the general scan).  digests, or
    expected + verdicts, may be None; with none of them the call only decodes."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_b64_verify_launch(p(text), p(text_offsets), p(text_lens), n, max_text_len, p(expected_sizes),
                                       max_size, p(out), p(out_offsets), p(out_sizes), p(digests), p(expected),
                                       p(verdicts), p(work), stream))


# hash_text.hpp's kMapBlock and kScanWidth: the chunks a workgroup of the
# chunkmap kernels takes, and the workgroup counts the scan takes a trip
HASH_TEXT_MAP_BLOCK = 1024
HASH_TEXT_SCAN_WIDTH = 1024


def verify_hashes_launch_work(n: int) -> int:
    """lbf_verify_hashes_launch_work: the bytes of `work` sha1_hashes_launch and
    verify_hashes_launch need for n chunks."""
    return int(load().lbf_verify_hashes_launch_work(n))


def sha1_hashes_launch(base, offsets, sizes, n, hashes, work, hash_offsets=None, digests=None, stream=None):
    """lbf_sha1_hashes_launch: chunks in device memory hashed and their
    27-character hash strings (the flood file's form, no NUL) written at
    hashes + hash_offsets[i], or packed at 27 * i when hash_offsets is None,
    asynchronous on `stream`; nothing outside the slots is written.  `work` is
    verify_hashes_launch_work(n) bytes; the digests land in `digests`, or in
    `work` when it is None."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_sha1_hashes_launch(p(base), p(offsets), p(sizes), n, p(hashes), p(hash_offsets), p(digests),
                                        p(work), stream))


def verify_hashes_launch(base, offsets, sizes, n, hashes, chunkmap, work, hash_offsets=None, hash_lens=None,
                         missing=None, missing_count=None, digests=None, stream=None):
    """lbf_verify_hashes_launch: chunks in device memory hashed and compared, as
    strings, with the flood file's hashes (hashes + hash_offsets[i], hash_lens[i]
    characters; both None for packed 27-character strings), asynchronous on
    `stream`.  chunkmap[i] = '1' for an equal string of length 27, else '0';
    missing[0, missing_count[0]) receives the indices with '0' in ascending
    order (both may be None).  `work` is verify_hashes_launch_work(n) bytes."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_verify_hashes_launch(p(base), p(offsets), p(sizes), n, p(hashes), p(hash_offsets), p(hash_lens),
                                          p(chunkmap), p(missing), p(missing_count), p(digests), p(work), stream))


# wire_frames.hpp's geometry: the bytes of the stream a workgroup of the split
# kernels takes, the bytes a trip of the locate kernel's search takes, the
# frames a workgroup of the bind kernels takes, the counts the scan takes a trip
WIRE_SPLIT_BLOCK = 4096
WIRE_SEARCH_TRIP = 4096
WIRE_BIND_BLOCK = 256
WIRE_SCAN_WIDTH = 1024
LBF_FRAME_OTHER, LBF_FRAME_SEND_CHUNK, LBF_FRAME_SEND_CHUNK_UNBOUND = 0, 1, 2
# lbf_wire_frame
WIRE_FRAME_DTYPE = np.dtype([("text_offset", "<u8"), ("name_offset", "<u8"), ("text_len", "<u4"), ("name_len", "<u4"),
                             ("index", "<u4"), ("kind", "<u4")])


def wire_frames_launch_work(stream_len: int) -> int:
    """lbf_wire_frames_launch_work: the bytes of `work` wire_frames_launch needs
    for a stream of stream_len bytes, 4 * ceil((stream_len + 15) / 4096)."""
    return int(load().lbf_wire_frames_launch_work(stream_len))


def wire_send_chunks_launch_work(n_frames: int) -> int:
    """lbf_wire_send_chunks_launch_work: the bytes of `work` wire_send_chunks_launch
    needs for n_frames frames, 4 * n_frames + 4 * ceil(n_frames / 256)."""
    return int(load().lbf_wire_send_chunks_launch_work(n_frames))


def wire_frames_launch(stream_buf, stream_len, frame_offsets, frame_lens, max_frames, n_frames, tail, work,
                       stream=None):
    """lbf_wire_frames_launch: the receive stream stream_buf[0, stream_len) in
    device memory split on '\\n', asynchronous on `stream`: the first max_frames
    frames to frame_offsets (uint64) / frame_lens (uint32), the number found to
    n_frames[0] (uint32), the start of the unfinished last frame to tail[0]
    (uint64).  frame_offsets and frame_lens may be None with max_frames == 0.
    `work` is wire_frames_launch_work(stream_len) bytes."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_wire_frames_launch(p(stream_buf), stream_len, p(frame_offsets), p(frame_lens), max_frames,
                                        p(n_frames), p(tail), p(work), stream))


def wire_send_chunks_launch(stream_buf, stream_len, frame_offsets, frame_lens, n_frames, frames, work,
                            live_frames=None, file_names=None, file_name_offsets=None, file_first=None, n_files=0,
                            chunk_sizes=None, chunk_expected=None, n_chunks=0, text_offsets=None, text_lens=None,
                            expected_sizes=None, expected=None, chunk_of=None, frame_of=None, max_chunks=0,
                            n_located=None, stream=None):
    """lbf_wire_send_chunks_launch: PeerWire::LocateSendChunk on every live frame
    of the stream in device memory (the first min(live_frames[0], n_frames), or
    n_frames when live_frames is None) into frames (WIRE_FRAME_DTYPE), bound to
    the flood table (wire_flood_table's five arrays, or none) and compacted into
    the dense tables verify_b64_launch reads (or none), asynchronous on
    `stream`.  `work` is wire_send_chunks_launch_work(n_frames) bytes."""
    p = lambda x: None if x is None else (x.ptr if isinstance(x, DeviceBuffer) else x)  # noqa: E731
    check(load().lbf_wire_send_chunks_launch(p(stream_buf), stream_len, p(frame_offsets), p(frame_lens), n_frames,
                                             p(live_frames), p(file_names), p(file_name_offsets), p(file_first),
                                             n_files, p(chunk_sizes), p(chunk_expected), n_chunks, p(frames),
                                             p(text_offsets), p(text_lens), p(expected_sizes), p(expected),
                                             p(chunk_of), p(frame_of), max_chunks, p(n_located), p(work), stream))


def xml_encode(name: bytes | str) -> bytes:
    """XmlRpcUtil::xmlEncode as PeerWire::XmlEncode has it: the five characters
    < > & ' " as their entities, every other byte as it is."""
    raw = name.encode() if isinstance(name, str) else bytes(name)
    ent = {ord("<"): b"&lt;", ord(">"): b"&gt;", ord("&"): b"&amp;", ord("'"): b"&apos;", ord('"'): b"&quot;"}
    return b"".join(ent.get(c, bytes([c])) for c in raw)


def wire_flood_table(files):
    """The flood table wire_send_chunks_launch binds against, from
    [(name, sizes, digests)] in the flood's order (digests: 20 bytes per chunk,
    as bytes objects or an (n, 20) array): (file_names uint8, file_name_offsets
    uint32[n_files + 1], file_first uint32[n_files + 1], chunk_sizes uint32,
    chunk_expected uint8[20 * n_chunks]), host arrays ready to upload."""
    names, name_off, first, sizes, digests = [], [0], [0], [], []
    for name, file_sizes, file_digests in files:
        file_sizes = [int(x) for x in file_sizes]
        file_digests = [bytes(bytearray(d)) for d in file_digests]
        if len(file_sizes) != len(file_digests) or any(len(d) != 20 for d in file_digests):
            raise ValueError("wire_flood_table: one 20-byte digest per chunk size")
        names.append(xml_encode(name))
        name_off.append(name_off[-1] + len(names[-1]))
        first.append(first[-1] + len(file_sizes))
        sizes += file_sizes
        digests += file_digests
    return (np.frombuffer(b"".join(names), np.uint8).copy(), np.array(name_off, np.uint32),
            np.array(first, np.uint32), np.array(sizes, np.uint32),
            np.frombuffer(b"".join(digests), np.uint8).copy())


def set_b64_lines(on) -> bool:
    """lbf_set_b64_lines: the line path of update_text / b64_update_launch on or
    off, process-wide; returns the previous setting."""
    return bool(load().lbf_set_b64_lines(1 if on else 0))


def set_b64_flat(on) -> bool:
    """lbf_set_b64_flat: the flat path (unbroken base64 text, as bitflood's Java
    and Perl peers send it) of verify_b64 / update_text / b64_update_launch on
    or off, process-wide; returns the previous setting."""
    return bool(load().lbf_set_b64_flat(1 if on else 0))


def set_b64_fused(on) -> bool:
    """lbf_set_b64_fused: the fused route of update_text / b64_update_launch (the
    line, flat and scan stages of a piece in one kernel launch, set_b64_lines
    and set_b64_flat as its stage mask) on or off, process-wide; returns the
    previous setting."""
    return bool(load().lbf_set_b64_fused(1 if on else 0))


def synchronize():
    check(load().lbf_device_synchronize())


def set_kernel_variant(v: int):
    check(load().lbf_set_kernel_variant(v))


__all__ = ["ChunkHasher", "DeviceBuffer", "LbfError", "b64_27", "b64_27_decode", "chunk_table",
           "uniform_launch", "batch_launch", "update_launch", "STATE_DTYPE", "new_states",
           "B64_STATE_DTYPE", "new_b64_states", "b64_update_launch", "B64_ENC_STATE_DTYPE", "new_b64_enc_states",
           "b64_text_length", "b64_encode_update_launch", "verify_encode_b64_launch",
           "verify_b64_launch", "b64_verify_launch_work",
           "sha1_hashes_launch", "verify_hashes_launch", "verify_hashes_launch_work",
           "HASH_TEXT_MAP_BLOCK", "HASH_TEXT_SCAN_WIDTH",
           "wire_frames_launch", "wire_frames_launch_work", "wire_send_chunks_launch", "wire_send_chunks_launch_work",
           "WIRE_FRAME_DTYPE", "WIRE_SPLIT_BLOCK", "WIRE_SEARCH_TRIP", "WIRE_BIND_BLOCK", "WIRE_SCAN_WIDTH",
           "LBF_FRAME_OTHER", "LBF_FRAME_SEND_CHUNK", "LBF_FRAME_SEND_CHUNK_UNBOUND", "xml_encode", "wire_flood_table",
           "chain_table", "update_seq_launch", "b64_update_seq_launch",
           "set_b64_lines", "set_b64_flat", "set_b64_fused", "synchronize", "set_kernel_variant", "LBF_DEVICE_PTR",
           "_capi"]

"""lbf_sha1_hashes_launch and lbf_verify_hashes_launch on the GPU: chunks
resident in device memory to and against the flood file's 27-character hash
strings, chunkmap and to-download list built on the device
(bitflood_amd/csrc/hash_text.hip).

The model of every comparison is the CPU: hashlib.sha1 and
base64.b64encode(d)[:27] (pinned against Crypto++'s own vector in
tests/test_abi.py), and a chunkmap character is '1' exactly when the given
bytes equal the model's string.  Every output array is prefilled (0xEE, or
0xFFFFFFFF for the list) and checked whole, so a byte written outside a slot,
or an entry written past the count, fails the case.
"""
import base64
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from bitflood_amd import DeviceBuffer, _capi
from bitflood_amd import hashing as H

pytestmark = pytest.mark.gpu

FILL = 0xEE
UNSET = 0xFFFFFFFF
SIZES = (0, 1, 55, 56, 63, 64, 65, 119, 120, 4096 + 1)
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
MAP_BLOCK, SCAN_WIDTH = H.HASH_TEXT_MAP_BLOCK, H.HASH_TEXT_SCAN_WIDTH


def model_string(chunk: bytes) -> bytes:
    return base64.b64encode(hashlib.sha1(chunk).digest())[:27]


class Scene:
    """n chunks packed back to back, with hashlib's digests and the model's strings."""

    def __init__(self, sizes, seed):
        rng = np.random.default_rng(seed)
        self.sizes = np.asarray(sizes, np.uint32)
        self.n = len(self.sizes)
        ends = np.cumsum(self.sizes, dtype=np.uint64)
        self.offs = (ends - self.sizes).astype(np.uint64)
        self.data = rng.integers(0, 256, int(ends[-1]) if self.n else 0, dtype=np.uint8)
        self.rehash()

    def chunk(self, i):
        return self.data[int(self.offs[i]):int(self.offs[i]) + int(self.sizes[i])].tobytes()

    def rehash(self):
        raw, at = self.data.tobytes(), self.offs.tolist()
        d = [hashlib.sha1(raw[a:a + s]).digest() for a, s in zip(at, self.sizes.tolist())]
        self.digests = np.frombuffer(b"".join(d), np.uint8).reshape(self.n, 20)
        self.strings = [base64.b64encode(x)[:27] for x in d]


@functools.lru_cache(maxsize=None)
def scene(n, seed=1):
    """The drawn sizes, every one of SIZES present once n allows it.  Shared and left unchanged."""
    rng = np.random.default_rng(1000 + seed)
    sizes = rng.choice(SIZES, n)
    sizes[:min(n, len(SIZES))] = SIZES[:min(n, len(SIZES))]
    return Scene(sizes, seed)


class Dev:
    """Device buffers of one test, freed together."""

    def __init__(self):
        self.bufs = []

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()

    def filled(self, nbytes, byte=FILL):
        return self.up(np.full(max(int(nbytes), 1), byte, np.uint8))

    def up(self, host):
        host = np.ascontiguousarray(host)
        b = DeviceBuffer(max(host.nbytes, 1))
        if host.nbytes:
            b.upload(host)
        self.bufs.append(b)
        return b

    def chunks(self, sc):
        return self.up(sc.data if sc.data.size else np.zeros(1, np.uint8)), self.up(sc.offs), self.up(sc.sizes)


def packed(strings):
    return np.frombuffer(b"".join(strings), np.uint8)


# ---------------------------------------------------------------------------
# sha1_hashes_launch
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2 * 256 + 3])
def test_hashes_packed_slots(n):
    sc = scene(n)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        out, work = d.filled(27 * n + 64), d.filled(H.verify_hashes_launch_work(n))
        H.sha1_hashes_launch(data, offs, sizes, n, out, work)
        H.synchronize()
        got = out.download()
    assert got[:27 * n].tobytes() == b"".join(sc.strings)
    assert (got[27 * n:] == FILL).all()


@pytest.mark.parametrize("phase", [1, 2, 3, 15])
def test_hashes_packed_slots_at_a_shifted_base(phase):
    n = 2 * 256 + 3
    sc = scene(n)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        out, work = d.filled(16 + 27 * n + 64), d.filled(H.verify_hashes_launch_work(n))
        assert out.ptr % 16 == 0
        H.sha1_hashes_launch(data, offs, sizes, n, out.ptr + phase, work)
        H.synchronize()
        got = out.download()
    assert (got[:phase] == FILL).all()
    assert got[phase:phase + 27 * n].tobytes() == b"".join(sc.strings)
    assert (got[phase + 27 * n:] == FILL).all()


def test_hashes_slot_offsets_at_every_phase_in_reversed_order():
    n = 257
    sc = scene(n)
    pitch = np.array([27 + (i % 5) for i in range(n)], np.uint64)
    place = np.cumsum(pitch) - pitch + np.uint64(5)  # slot k of the arena, in address order
    hoff = place[::-1].copy()  # chunk i takes slot n - 1 - i
    assert {int(o) % 16 for o in hoff} == set(range(16)) and {int(o) % 4 for o in hoff} == set(range(4))
    total = int(place[-1]) + 27 + 64
    want = np.full(total, FILL, np.uint8)
    for i in range(n):
        want[int(hoff[i]):int(hoff[i]) + 27] = np.frombuffer(sc.strings[i], np.uint8)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        out, work = d.filled(total), d.filled(H.verify_hashes_launch_work(n))
        H.sha1_hashes_launch(data, offs, sizes, n, out, work, hash_offsets=d.up(hoff))
        H.synchronize()
        got = out.download()
    assert np.array_equal(got, want)  # every slot exact, every byte between slots untouched


def test_hashes_digests_given_or_not():
    n = 257
    sc = scene(n)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        a, b = d.filled(27 * n), d.filled(27 * n)
        dig, work = d.filled(20 * n), d.filled(H.verify_hashes_launch_work(n))
        H.sha1_hashes_launch(data, offs, sizes, n, a, work, digests=dig)
        H.synchronize()
        work_after = work.download()
        H.sha1_hashes_launch(data, offs, sizes, n, b, work)
        H.synchronize()
        assert np.array_equal(dig.download().reshape(n, 20), sc.digests)
        assert (work_after[:20 * n] == FILL).all()  # the digests went where the caller asked
        assert a.download().tobytes() == b"".join(sc.strings) == b.download().tobytes()
        assert np.array_equal(work.download(20 * n).reshape(n, 20), sc.digests)


def test_hashes_under_a_producer_consumer_hash_kernel():
    n = 300
    if _capi.load().lbf_kernel_for(n) == 1:
        pytest.skip("300 chunks select the lane kernel under the current setting")
    assert _capi.load().lbf_kernel_for(n) != 1
    sc = Scene(np.full(n, 65536, np.uint32), seed=9)
    given = list(sc.strings)
    given[7] = given[8]
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        out, work = d.filled(27 * n + 64), d.filled(H.verify_hashes_launch_work(n))
        cmap, miss, cnt = d.filled(n), d.filled(4 * n, 0xFF), d.filled(4)
        H.sha1_hashes_launch(data, offs, sizes, n, out, work)
        H.verify_hashes_launch(data, offs, sizes, n, d.up(packed(given)), cmap, work, missing=miss, missing_count=cnt)
        H.synchronize()
        got = out.download()
        assert got[:27 * n].tobytes() == b"".join(sc.strings) and (got[27 * n:] == FILL).all()
        assert cmap.download().tobytes() == b"1" * 7 + b"0" + b"1" * (n - 8)
        assert cnt.download(dtype=np.uint32)[0] == 1 and miss.download(dtype=np.uint32)[0] == 7


# ---------------------------------------------------------------------------
# verify_hashes_launch
# ---------------------------------------------------------------------------
def lay_out(given, mixed):
    """The given strings in a 0xEE arena: packed (no tables), or one after another with 0-4 bytes between."""
    if not mixed:
        return packed(given), None, None
    hoff, cur = np.zeros(len(given), np.uint64), 3
    for i, g in enumerate(given):
        hoff[i] = cur
        cur += len(g) + (i % 5)
    text = np.full(cur + 32, FILL, np.uint8)
    for i, g in enumerate(given):
        text[int(hoff[i]):int(hoff[i]) + len(g)] = np.frombuffer(g, np.uint8)
    return text, hoff, np.array([len(g) for g in given], np.uint32)


def model_map(sc, given):
    return np.frombuffer(b"".join(b"1" if g == s else b"0" for g, s in zip(given, sc.strings)), np.uint8)


def run_verify(sc, given, mixed=False, with_list=True, with_digests=False, stream=None, d=None):
    """One launch with fresh, prefilled outputs; returns (chunkmap, count or None, missing or None, digests or None)."""
    n = sc.n
    own = d is None
    d = Dev() if own else d
    try:
        data, offs, sizes = d.chunks(sc)
        text, hoff, hlen = lay_out(given, mixed)
        cmap, work = d.filled(n), d.filled(H.verify_hashes_launch_work(n))
        miss, cnt = (d.filled(4 * n, 0xFF), d.filled(4)) if with_list else (None, None)
        dig = d.filled(20 * n) if with_digests else None
        H.verify_hashes_launch(data, offs, sizes, n, d.up(text), cmap, work,
                               hash_offsets=None if hoff is None else d.up(hoff),
                               hash_lens=None if hlen is None else d.up(hlen), missing=miss, missing_count=cnt,
                               digests=dig, stream=stream)
        if stream is not None:
            return cmap, cnt, miss, dig  # the caller synchronises and downloads
        H.synchronize()
        return (cmap.download(n), None if cnt is None else int(cnt.download(dtype=np.uint32)[0]),
                None if miss is None else miss.download(4 * n, dtype=np.uint32),
                None if dig is None else dig.download(20 * n).reshape(n, 20))
    finally:
        if own:
            d.__exit__()


def check_against_model(sc, given, got, want=None):
    cmap, count, missing, _ = got
    want = model_map(sc, given) if want is None else want
    assert cmap.tobytes() == want.tobytes()
    bad = np.flatnonzero(want == ord("0"))
    assert count == len(bad)
    assert np.array_equal(missing[:count], bad)
    assert (missing[count:] == UNSET).all()


@pytest.mark.parametrize("n", [1, 1023, 1024, 1025, 2 * 1024 + 1])
def test_verify_all_good(n):
    sc = scene(n)
    cmap, count, missing, _ = run_verify(sc, sc.strings)
    assert cmap.tobytes() == b"1" * n
    assert count == 0
    assert (missing == UNSET).all()


def damaged(sc, i, kind):
    """Chunk i's string damaged one way (the scene itself is not touched)."""
    s = bytearray(sc.strings[i])
    other = lambda c: ord("A") if c != ord("A") else ord("B")  # noqa: E731
    if kind in ("pos0", "pos13", "pos26"):
        p = int(kind[3:])
        s[p] = other(s[p])
    elif kind in ("low1", "low2", "low3"):
        v = ALPHABET.index(bytes([s[26]]))
        assert v % 4 == 0
        s[26] = ALPHABET[v + int(kind[3:])]  # shares the top four bits; the low two are not zero
    elif kind == "len26":
        del s[26]
    elif kind == "len28":
        s.append(ord("A"))
    elif kind == "len0":
        s = bytearray()
    elif kind in ("eq", "space", "x80"):
        s[13] = {"eq": ord("="), "space": ord(" "), "x80": 0x80}[kind]
    elif kind == "swap":
        j = (i + 7) % sc.n
        while sc.strings[j] == sc.strings[i]:  # two empty chunks share a hash
            j = (j + 1) % sc.n
        s = bytearray(sc.strings[j])
    else:
        raise AssertionError(kind)
    return bytes(s)


KINDS = ("pos0", "pos13", "pos26", "low1", "low2", "low3", "len26", "len28", "len0", "eq", "space", "x80", "swap",
         "bitflip")


def test_verify_every_damage_kind_across_wave_and_workgroup_boundaries():
    n = 2 * 1024 + 1
    base = scene(n)
    sc = Scene(base.sizes, seed=1)  # a copy of its own: the bit flips change the data
    assert np.array_equal(sc.data, base.data)
    where = sorted(set([0, 63, 64, 1023, 1024, 2047, 2048]) | set(range(990, 1060)))
    assert len(where) == 75 and len(range(990, 1060)) == 70
    given = list(sc.strings)
    for k, i in enumerate(where):
        kind = KINDS[k % len(KINDS)]
        if kind == "bitflip":  # the flood file's (correct) string for data that has since lost a bit
            if sc.sizes[i] == 0:
                kind = "pos13"
            else:
                sc.data[int(sc.offs[i]) + int(sc.sizes[i]) // 2] ^= 0x10
                continue
        given[i] = damaged(sc, i, kind)
    sc.rehash()
    want = model_map(sc, given)
    assert np.array_equal(np.flatnonzero(want == ord("0")), where)  # every kind reads as not verified
    check_against_model(sc, given, run_verify(sc, given, mixed=True), want)


def test_verify_every_chunk_damaged():
    n = 1025
    sc = scene(n)
    given = [damaged(sc, i, KINDS[i % 13]) for i in range(n)]
    got = run_verify(sc, given, mixed=True)
    check_against_model(sc, given, got)
    assert got[1] == n and np.array_equal(got[2], np.arange(n))


def test_verify_only_the_last_chunk_damaged():
    n = 2049
    sc = scene(n)
    given = list(sc.strings)
    given[-1] = damaged(sc, n - 1, "low2")
    got = run_verify(sc, given)
    check_against_model(sc, given, got)
    assert got[1] == 1 and got[2][0] == n - 1


def test_verify_without_the_list_and_with_digests():
    n = 1025
    sc = scene(n)
    given = [damaged(sc, i, "pos26") if i % 3 == 0 else sc.strings[i] for i in range(n)]
    want = model_map(sc, given)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        text = d.up(packed(given))
        cmap, work = d.filled(n + 64), d.filled(H.verify_hashes_launch_work(n) + 64)
        H.verify_hashes_launch(data, offs, sizes, n, text, cmap, work)
        H.synchronize()
        got, w = cmap.download(), work.download()
        assert got[:n].tobytes() == want.tobytes() and (got[n:] == FILL).all()
        assert np.array_equal(w[:20 * n].reshape(n, 20), sc.digests)  # no d_digests: the hash writes into d_work
        assert (w[20 * n:] == FILL).all()  # no list: no counts, nothing else
    a = run_verify(sc, given, with_digests=True)
    b = run_verify(sc, given, with_list=False, with_digests=True)
    for got in (a, b):
        assert got[0].tobytes() == want.tobytes()
        assert np.array_equal(got[3], sc.digests)
    check_against_model(sc, given, a, want)


@functools.lru_cache(maxsize=None)
def big_scene():
    n = SCAN_WIDTH * MAP_BLOCK + MAP_BLOCK + 1
    rng = np.random.default_rng(77)
    return Scene(rng.integers(1, 4, n).astype(np.uint32), seed=77)


def test_verify_scan_of_more_than_one_trip():
    sc = big_scene()
    n = sc.n
    assert H.verify_hashes_launch_work(n) == ((20 * n + 15) & ~15) + 4 * (SCAN_WIDTH + 2)  # two trips of the scan
    second = SCAN_WIDTH * MAP_BLOCK  # the first chunk whose workgroup count the second trip takes
    given = list(sc.strings)
    same_length = [k for k in KINDS[:13] if not k.startswith("len")]  # packed strings: 27 characters each
    for i in sorted(set(range(0, n, 997)) | {second, n - 1}):
        given[i] = damaged(sc, i, same_length[i % len(same_length)])
    check_against_model(sc, given, run_verify(sc, given))


def test_verify_two_streams_with_separate_work_and_outputs():
    lib = _capi.load()
    n = 2049
    sc = scene(n)
    givens = ([damaged(sc, i, "pos0") if i % 5 == 0 else sc.strings[i] for i in range(n)],
              [damaged(sc, i, "len26") if i % 7 == 3 else sc.strings[i] for i in range(n)])
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for s in streams:
        _capi.check(lib.lbf_stream_create(ctypes.byref(s)))
    try:
        with Dev() as d:
            outs = [run_verify(sc, g, mixed=(k == 1), stream=s, d=d) for k, (g, s) in enumerate(zip(givens, streams))]
            for s in streams:
                _capi.check(lib.lbf_stream_synchronize(s))
            for g, (cmap, cnt, miss, _) in zip(givens, outs):
                check_against_model(sc, g, (cmap.download(n), int(cnt.download(dtype=np.uint32)[0]),
                                            miss.download(4 * n, dtype=np.uint32), None))
    finally:
        for s in streams:
            _capi.check(lib.lbf_stream_destroy(s))


def test_verify_relaunch_into_the_same_buffers_carries_no_state():
    n = 2049
    sc = scene(n)
    first = [damaged(sc, i, "pos13") if i % 2 == 0 else sc.strings[i] for i in range(n)]
    then = [damaged(sc, i, "eq") if i in (5, 1024, 2048) else sc.strings[i] for i in range(n)]
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        text = d.up(packed(first))
        cmap, work = d.filled(n), d.filled(H.verify_hashes_launch_work(n))
        miss, cnt = d.filled(4 * n, 0xFF), d.filled(4)
        for given in (first, then):
            text.upload(packed(given))
            miss.upload(np.full(n, UNSET, np.uint32))
            H.verify_hashes_launch(data, offs, sizes, n, text, cmap, work, missing=miss, missing_count=cnt)
            H.synchronize()
            check_against_model(sc, given, (cmap.download(n), int(cnt.download(dtype=np.uint32)[0]),
                                            miss.download(4 * n, dtype=np.uint32), None))


def test_round_trip_device_to_device():
    n = 2 * 1024 + 1
    sc = scene(n)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        text, work = d.filled(27 * n), d.filled(H.verify_hashes_launch_work(n))
        cmap, miss, cnt = d.filled(n), d.filled(4 * n, 0xFF), d.filled(4)
        H.sha1_hashes_launch(data, offs, sizes, n, text, work)
        H.verify_hashes_launch(data, offs, sizes, n, text, cmap, work, missing=miss, missing_count=cnt)
        H.synchronize()
        assert cmap.download(n).tobytes() == b"1" * n
        assert cnt.download(dtype=np.uint32)[0] == 0 and (miss.download(dtype=np.uint32) == UNSET).all()


def test_a_table_too_short_for_its_allocation_is_refused():
    lib = _capi.load()
    n = 64
    sc = scene(n)
    with Dev() as d:
        data, offs, sizes = d.chunks(sc)
        text, work, cmap = d.up(packed(sc.strings)), d.filled(H.verify_hashes_launch_work(n)), d.filled(n)
        short = d.filled(27 * n - 1)
        with pytest.raises(H.LbfError, match=r"lbf_sha1_hashes_launch: hashes: .*past its allocation"):
            H.sha1_hashes_launch(data, offs, sizes, n, short, work)
        with pytest.raises(H.LbfError, match=r"lbf_verify_hashes_launch: chunkmap: .*past its allocation"):
            H.verify_hashes_launch(data, offs, sizes, n, text, d.filled(n - 1), work)
        with pytest.raises(H.LbfError, match=r"lbf_verify_hashes_launch: work: .*past its allocation"):
            H.verify_hashes_launch(data, offs, sizes, n, text, cmap, d.filled(20 * n))
        assert lib.lbf_device_synchronize() == 0
        assert (short.download() == FILL).all() and (cmap.download() == FILL).all()  # nothing was enqueued

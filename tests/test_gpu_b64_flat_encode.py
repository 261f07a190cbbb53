"""Chunks to send verified and encoded in one shot, in either peer's text
layout, from host memory (lbf_verify_encode_b64_layout_batch,
ChunkHasher.verify_encode_b64) and from device memory
(lbf_verify_encode_b64_launch): xmlrpc++'s lines through the line kernel, the
Java and Perl peers' unbroken text through b64_flat_encode_kernel
(bitflood_amd/csrc/b64_flat_encode.hip).

Expected values never come from the code under test: base64.b64encode for
unbroken text, tests/wire_layouts.xmlrpc_text (pinned to xmlrpc++'s recorded
encoder output) for lines, hashlib.sha1 for digests.  Sizes come from
tests/wire_flat_encode_model.py (T = tile bytes, K = tiles per workgroup).
Every call is checked whole: a 0xA5-filled text arena must hold each chunk's
text in its slot and 0xA5 everywhere else.
"""
import functools
import hashlib
import math

import numpy as np
import pytest

from bitflood_amd import DeviceBuffer, LbfError, _capi, new_b64_enc_states, new_states
from bitflood_amd import hashing as H
from tests import large_index as L
from tests import wire_flat_encode_model as F

pytestmark = pytest.mark.gpu

FILL = 0xA5
T, K = F.T, F.K
BOTH = ("xmlrpc", "flat")
VIAS = ("batch", "launch")


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


class Batch:
    """Chunks of the given sizes laid into a data arena and a text arena.
    dphase / tphase: the residues mod 16 of chunk i's bytes and of its slot
    (None: wherever the gaps put them); gap(i) = the bytes left free in front
    of slot i (0: it touches slot i - 1).  `want` is the text arena as it must
    look afterwards."""

    def __init__(self, sizes, layout, seed, dphase=None, tphase=None, gap=lambda i: 1 + i % 3):
        self.layout, self.lay = layout, F.LAYOUTS[layout]
        n = len(sizes)
        self.n = n
        self.sizes = np.array(sizes, dtype=np.uint32)
        rng = np.random.default_rng(seed)
        self.offs = np.zeros(n, dtype=np.uint64)
        pos = 16
        for i, s in enumerate(sizes):
            pos += i % 2
            if dphase is not None:
                pos += (dphase[i] - pos) % 16
            self.offs[i] = pos
            pos += s
        self.data = rng.integers(0, 256, pos + 16, dtype=np.uint8)
        self.chunks = [self.data[int(o):int(o) + int(s)].tobytes() for o, s in zip(self.offs, self.sizes)]
        self.texts = [F.text(c, self.lay) for c in self.chunks]
        self.lens = [len(t) for t in self.texts]
        self.toffs = np.zeros(n, dtype=np.uint64)
        pos = 16
        for i in range(n):
            pos += gap(i)
            if tphase is not None:
                pos += (tphase[i] - pos) % 16
            self.toffs[i] = pos
            pos += self.lens[i]
        self.want = np.full(pos + 48, FILL, dtype=np.uint8)
        for o, t in zip(self.toffs.tolist(), self.texts):
            self.want[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
        self.digests = np.frombuffer(b"".join(sha1(c) for c in self.chunks), dtype=np.uint8).reshape(n, 20).copy()
        self.expected = self.digests.copy()
        self.verdicts = np.ones(n, dtype=np.uint8)

    def flip(self, i):
        """Chunk i's expected digest off by a bit: verdict 0, its text written all the same."""
        self.expected[i, 7] ^= 0x10
        self.verdicts[i] = 0

    def where(self, at):
        i = max(int(np.searchsorted(self.toffs, int(at), side="right")) - 1, 0)
        return (f"text byte {int(at)}: slot {i} ({int(self.sizes[i])} B, {self.lens[i]} characters) "
                f"+ {int(at) - int(self.toffs[i])}")

    def check_text(self, got, what=""):
        wrong = np.flatnonzero(got != self.want)
        assert wrong.size == 0, (what, self.layout, wrong.size, self.where(wrong[0]))


def raw_batch(hasher, b, layout=None, data_len=None, text_len=None, sizes=None, toffs=None, offs=None, old=False):
    """One raw call of the batch entry over b's arenas; (rc, verdicts, text)."""
    lib = _capi.load()
    text = np.full(b.want.size, FILL, dtype=np.uint8)
    ver = np.full(b.n, FILL, dtype=np.uint8)
    sizes = b.sizes if sizes is None else np.ascontiguousarray(sizes, dtype=np.uint32)
    toffs = b.toffs if toffs is None else np.ascontiguousarray(toffs, dtype=np.uint64)
    offs = b.offs if offs is None else np.ascontiguousarray(offs, dtype=np.uint64)
    head = (hasher._h, b.data.ctypes.data, b.data.size if data_len is None else data_len, offs.ctypes.data,
            sizes.ctypes.data, b.n, b.expected.ctypes.data, ver.ctypes.data)
    tail = (text.ctypes.data, text.size if text_len is None else text_len, toffs.ctypes.data)
    if old:
        rc = lib.lbf_verify_encode_b64_batch(*head, *tail)
    else:
        rc = lib.lbf_verify_encode_b64_layout_batch(*head, b.lay if layout is None else layout, *tail)
    return rc, ver, text


class Launch:
    """b's arenas and tables in device memory, for lbf_verify_encode_b64_launch."""

    def __init__(self, b, room=8):
        self.b, self.room = b, room
        self.bufs = {}
        n = b.n
        for name, a in (("data", b.data), ("offs", b.offs), ("sizes", b.sizes), ("toffs", b.toffs),
                        ("exp", b.expected), ("text", np.full(b.want.size, FILL, dtype=np.uint8)),
                        ("dig", np.full(20 * (n + room), FILL, dtype=np.uint8)),
                        ("ver", np.full(n + room, FILL, dtype=np.uint8))):
            self.bufs[name] = DeviceBuffer(max(a.nbytes, 16))
            self.bufs[name].upload(a)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for buf in self.bufs.values():
            buf.free()

    def run(self, max_size=None, digests=True, verdicts=True, layout=None, **over):
        d = dict(self.bufs, **over)
        b = self.b
        H.verify_encode_b64_launch(d["data"], d["offs"], d["sizes"], b.n,
                                   int(b.sizes.max()) if max_size is None else max_size, d["text"], d["toffs"],
                                   layout=b.layout if layout is None else layout, digests=d["dig"] if digests else None,
                                   expected=d["exp"] if verdicts else None, verdicts=d["ver"] if verdicts else None)
        H.synchronize()
        return self.results()

    def results(self):
        n, room = self.b.n, self.room
        dig = self.bufs["dig"].download(20 * (n + room)).reshape(-1, 20)
        ver = self.bufs["ver"].download(n + room)
        return dig, ver, self.bufs["text"].download(self.b.want.size)

    def untouched(self):
        dig, ver, text = self.results()
        return bool((dig == FILL).all() and (ver == FILL).all() and (text == FILL).all())


def run(hasher, b, via):
    """The batch through either entry, everything checked: the whole text
    arena, the verdicts and (the launch) the digests and the guard entries."""
    if via == "batch":
        rc, ver, text = raw_batch(hasher, b)
        assert rc == 0, _capi.load().lbf_last_error()
        b.check_text(text, via)
        assert np.array_equal(ver, b.verdicts), np.flatnonzero(ver != b.verdicts)[:8].tolist()
        return text
    with Launch(b) as dev:
        dig, ver, text = dev.run()
        b.check_text(text, via)
        bad = np.flatnonzero(ver[:b.n] != b.verdicts)
        assert bad.size == 0, ("verdicts", bad[:8].tolist())
        bad = np.flatnonzero((dig[:b.n] != b.digests).any(axis=1))
        assert bad.size == 0, ("digests", bad[:8].tolist())
        assert (dig[b.n:] == FILL).all() and (ver[b.n:] == FILL).all(), "entries past the last chunk written"
        return text


# ------------------------------------------------------------------ 1. sizes
@functools.lru_cache(maxsize=None)
def sizes_batch(layout):
    sizes = F.sizes_for(F.LAYOUTS[layout])
    n = len(sizes)
    b = Batch(sizes, layout, seed=1, dphase=[(5 * i + 3) % 16 for i in range(n)])
    b.flip(sizes.index(K * T + 1))
    return b


@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_sizes(hasher, layout, via):
    """Every size of the model in one batch -- the last group's three forms
    below and above a block and a line, both sides of the tile and of the
    workgroup, a chunk of more than two workgroups; for lines the sizes of
    wire_layouts.encode_cases() too -- at rotating source phases, the slots at
    whatever phase the lengths and gaps of 1 to 3 bytes give.  One expected
    digest is off by a bit: verdict 0, and the text still written."""
    b = sizes_batch(layout)
    assert 0 in b.sizes and b.verdicts.sum() == b.n - 1
    run(hasher, b, via)


def test_python_binding(hasher):
    """ChunkHasher.verify_encode_b64 with a layout; the default is lines."""
    b = sizes_batch("flat")
    ver, texts = hasher.verify_encode_b64(b.data, b.offs, b.sizes, b.expected, layout="flat")
    assert texts == b.texts and np.array_equal(ver, b.verdicts.astype(bool))
    x = sizes_batch("xmlrpc")
    ver, texts = hasher.verify_encode_b64(x.data, x.offs, x.sizes, x.expected)
    assert texts == x.texts and np.array_equal(ver, x.verdicts.astype(bool))
    with pytest.raises(ValueError):
        hasher.verify_encode_b64(b.data, b.offs, b.sizes, b.expected, layout="lines")


# ----------------------------------------------------------------- 2. phases
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_every_pair_of_phases(hasher, layout, via):
    """256 chunks of T + 1 bytes whose bytes and slots start at every pair of
    residues mod 16.  Touching slots of one length step through 16 / g
    residues, g = gcd(length, 16): g runs of 256 / g touching slots, one free
    byte in front of each run, reach all sixteen, and within a run the source
    phase moves on once the slot phases have come round."""
    step = F.text_length(T + 1, F.LAYOUTS[layout]) % 16
    g = math.gcd(step, 16)
    n, run_len, period = 256, 256 // g, 16 // g
    dphase = [(j % run_len) // period for j in range(n)]
    b = Batch([T + 1] * n, layout, seed=2, dphase=dphase, gap=lambda j: 1 if j % run_len == 0 else 0)
    pairs = {(int(o) % 16, int(t) % 16) for o, t in zip(b.offs, b.toffs)}
    assert len(pairs) == 256
    touching = sum(int(b.toffs[j]) == int(b.toffs[j - 1]) + b.lens[j - 1] for j in range(1, n))
    assert touching == n - g
    run(hasher, b, via)


# ----------------------------------------------------------------- 3. counts
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
@pytest.mark.parametrize("n", [1, 65, 300])
def test_counts(hasher, n, layout, via):
    rng = np.random.default_rng(30 + n)
    sizes = rng.choice([0, 1, 2, 3, 17, 53, 54, 55, 100, 161, 162, 1000, T + 5], n).tolist()
    if n == 1:
        sizes = [163]
    b = Batch(sizes, layout, seed=3 + n, gap=lambda i: i % 2)
    if n > 1:
        b.flip(n // 2)
    run(hasher, b, via)


@pytest.mark.parametrize("layout", BOTH)
def test_more_chunks_than_one_launch_takes(hasher, layout):
    """65,537 chunks of 1 to 50 bytes through the launch, slots touching: the
    encode goes out in two launches of grid.y <= 65,535, and flips stand on both
    sides of the split."""
    n = F.CHUNKS_PER_LAUNCH + 2
    sizes = np.random.default_rng(65).integers(1, 51, n).tolist()
    b = Batch(sizes, layout, seed=66, gap=lambda i: 0)
    for i in (0, F.CHUNKS_PER_LAUNCH - 1, F.CHUNKS_PER_LAUNCH, n - 1):
        b.flip(i)
    run(hasher, b, "launch")


# ------------------------------------------------------ 4. offsets past 4 GiB
@pytest.fixture(scope="module")
def big_pair():
    """Two allocations of 4 GiB + 1 MiB: the bytes (read) and the text (written)."""
    bufs = [DeviceBuffer(L.LINE + (1 << 20)), DeviceBuffer(L.LINE + (1 << 20))]
    try:
        yield bufs
    finally:
        for b in bufs:
            b.free()


@pytest.mark.parametrize("layout", BOTH)
def test_offsets_past_4_gib(layout, big_pair):
    """One chunk of more than one workgroup and its slot past byte 2^32 of their
    allocations, through the launch.  The positions minus 2^32 hold other bytes
    (data) or the fill (text), so an offset kept in 32 bits gives a wrong text or
    a written alias inside the allocation, never a fault."""
    big_data, big_text = big_pair
    lay = F.LAYOUTS[layout]
    size = K * T + 100
    rng = np.random.default_rng(40)
    doff, toff = L.LINE + 4096 + 5, L.LINE + 8192 + 11
    chunk = rng.integers(0, 256, size, dtype=np.uint8)
    want = F.text(chunk.tobytes(), lay)
    span = (len(want) + 15) // 16 * 16 + 64
    big_data.upload(rng.integers(0, 256, size + 64, dtype=np.uint8), doff - L.LINE - 16)   # the alias: other bytes
    big_data.upload(chunk, doff)
    fill = np.full(span, FILL, dtype=np.uint8)
    big_text.upload(fill, toff - L.LINE - 32)
    big_text.upload(fill, toff - 32)
    tabs = [DeviceBuffer(16) for _ in range(4)]
    try:
        d_off, d_size, d_toff, d_ver = tabs
        d_off.upload(np.array([doff], dtype=np.uint64))
        d_size.upload(np.array([size], dtype=np.uint32))
        d_toff.upload(np.array([toff], dtype=np.uint64))
        d_exp = DeviceBuffer(20)
        tabs.append(d_exp)
        d_exp.upload(np.frombuffer(sha1(chunk), dtype=np.uint8))
        d_ver.upload(np.full(16, FILL, dtype=np.uint8))
        H.verify_encode_b64_launch(big_data, d_off, d_size, 1, size, big_text, d_toff, layout=layout, expected=d_exp,
                                   verdicts=d_ver)
        H.synchronize()
        got = big_text.download(span, toff - 32)
        expect = fill.copy()
        expect[32:32 + len(want)] = np.frombuffer(want, dtype=np.uint8)
        wrong = np.flatnonzero(got != expect)
        assert wrong.size == 0, ("first wrong byte at slot %+d" % (int(wrong[0]) - 32), wrong.size)
        assert (big_text.download(span, toff - L.LINE - 32) == FILL).all(), "the slot's position mod 2^32 written"
        assert d_ver.download(16).tolist() == [1] + [FILL] * 15
    finally:
        for t in tabs:
            t.free()


# --------------------------------------------------------------- 5. max_size
@pytest.mark.parametrize("layout", BOTH)
def test_a_chunk_larger_than_max_size(hasher, layout):
    """max_size sizes the grid.  A chunk larger than it keeps what the contract
    promises: verdict 0, an incomplete text -- every character that is there is
    right -- and nothing written outside its slot; its neighbours are whole."""
    sizes = [100, 1000, 3 * K * T + 7, 999, 0, 1000]
    big = 2
    b = Batch(sizes, layout, seed=5, gap=lambda i: 0 if i in (2, 3) else 2)
    with Launch(b) as dev:
        dig, ver, text = dev.run(max_size=1000)
    lo, hi = int(b.toffs[big]), int(b.toffs[big]) + b.lens[big]
    outside = np.ones(text.size, dtype=bool)
    outside[lo:hi] = False
    wrong = np.flatnonzero((text != b.want) & outside)
    assert wrong.size == 0, b.where(wrong[0])
    slot, want = text[lo:hi], b.want[lo:hi]
    written = slot != FILL
    assert (slot[written] == want[written]).all(), "a wrong character in the oversize chunk's slot"
    assert not written.all(), "max_size = 1000 launched every tile of a chunk of three workgroups and more"
    want_ver = b.verdicts.copy()
    want_ver[big] = 0
    assert np.array_equal(ver[:b.n], want_ver) and (ver[b.n:] == FILL).all()
    assert np.array_equal(dig[:b.n], b.digests), "the digests are the bytes' whatever max_size says"
    # without verdicts nothing is there to clear: the call only encodes
    with Launch(b) as dev:
        dig, ver, text2 = dev.run(max_size=1000, digests=False, verdicts=False)
        assert (dig == FILL).all() and (ver == FILL).all()
        assert np.array_equal(text2, text)


def test_encode_only(hasher):
    """d_digests, d_expected and d_verdicts all NULL: the text alone."""
    for layout in BOTH:
        b = sizes_batch(layout)
        with Launch(b) as dev:
            dig, ver, text = dev.run(digests=False, verdicts=False)
        b.check_text(text, "encode only")
        assert (dig == FILL).all() and (ver == FILL).all()


# --------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("layout", BOTH)
def test_batch_refusals(hasher, layout):
    lib = _capi.load()
    b = Batch([100, 200, 300, 50], layout, seed=6)

    def refused(word, **kw):
        rc, ver, text = raw_batch(hasher, b, **kw)
        msg = lib.lbf_last_error()
        assert rc == _capi.LBF_ERR_INVALID and word in msg and b"lbf_verify_encode_b64_layout_batch" in msg, (rc, msg)
        assert (ver == FILL).all() and (text == FILL).all(), "outputs written by a refused call"

    toffs = b.toffs.copy()
    toffs[2] = toffs[1] + b.lens[1] - 1          # slot 2 starts on slot 1's last character
    refused(b"overlaps", toffs=toffs)
    refused(b"chunk 3 outside the buffer", data_len=int(b.offs[3]) + int(b.sizes[3]) - 1)
    offs = b.offs.copy()
    offs[1] = b.data.size + 1
    refused(b"chunk 1 outside the buffer", offs=offs)
    refused(b"text slot 3 outside the buffer", text_len=int(b.toffs[3]) + b.lens[3] - 1)
    refused(b"layout", layout=2)
    # a chunk over 1 GiB: the sizes table only, the buffers stay small
    sizes = b.sizes.copy()
    sizes[0] = (1 << 30) + 1
    refused(b"1 GiB", sizes=sizes, data_len=4 << 30, text_len=8 << 30)
    # and the same arenas, untouched by the refusals, go through
    rc, ver, text = raw_batch(hasher, b)
    assert rc == 0 and np.array_equal(text, b.want) and ver.all()


@pytest.mark.parametrize("layout", BOTH)
def test_launch_refusals(hasher, layout):
    b = Batch([100, 200, 300, 50], layout, seed=7)
    with Launch(b) as dev:
        short8, short4 = DeviceBuffer(8 * (b.n - 1)), DeviceBuffer(4 * (b.n - 1))
        try:
            short8.upload(b.toffs[:-1])
            short4.upload(b.sizes[:-1])
            for over, word in (({"offs": short8}, "offsets"), ({"toffs": short8}, "text_offsets"),
                               ({"sizes": short4}, "sizes"), ({"ver": short4.ptr + 4 * (b.n - 1) - 3}, "verdicts")):
                with pytest.raises(LbfError) as e:
                    dev.run(**over)
                assert e.value.status == _capi.LBF_ERR_INVALID and word in str(e.value), str(e.value)
                assert "lbf_verify_encode_b64_launch" in str(e.value) and "allocation" in str(e.value)
                assert dev.untouched()
            for over in ({"offs": dev.bufs["offs"].ptr + 4}, {"toffs": dev.bufs["toffs"].ptr + 2},
                         {"sizes": dev.bufs["sizes"].ptr + 2}):
                with pytest.raises(LbfError) as e:
                    dev.run(**over)
                assert e.value.status == _capi.LBF_ERR_INVALID and "aligned" in str(e.value), str(e.value)
                assert dev.untouched()
            for kw, word in (({"layout": 2}, "layout"), ({"max_size": (1 << 30) + 1}, "1 GiB")):
                with pytest.raises((LbfError, ValueError)) as e:
                    dev.run(**kw)
                assert word in str(e.value), str(e.value)
                assert dev.untouched()
            with pytest.raises(LbfError) as e:   # expected without verdicts
                H.verify_encode_b64_launch(dev.bufs["data"], dev.bufs["offs"], dev.bufs["sizes"], b.n, 300,
                                           dev.bufs["text"], dev.bufs["toffs"], layout=layout, expected=dev.bufs["exp"])
            assert e.value.status == _capi.LBF_ERR_INVALID and "go together" in str(e.value)
            assert dev.untouched()
            # n == 0 enqueues nothing, whatever the tables hold
            H.verify_encode_b64_launch(dev.bufs["data"], dev.bufs["offs"], dev.bufs["sizes"], 0, 300, dev.bufs["text"],
                                       dev.bufs["toffs"], layout=layout, digests=dev.bufs["dig"])
            H.synchronize()
            assert dev.untouched()
            # and the same tables, whole, go through
            dig, ver, text = dev.run()
            b.check_text(text, "after the refusals")
        finally:
            short8.free()
            short4.free()


# ----------------------------------------------------------- 7. equivalences
def test_lines_through_the_new_call_are_the_old_calls(hasher):
    """lbf_verify_encode_b64_layout_batch with LBF_B64_LAYOUT_XMLRPC against
    lbf_verify_encode_b64_batch, byte for byte over the whole arena."""
    b = sizes_batch("xmlrpc")
    rc_old, ver_old, text_old = raw_batch(hasher, b, old=True)
    rc_new, ver_new, text_new = raw_batch(hasher, b)
    assert rc_old == 0 and rc_new == 0
    assert np.array_equal(text_old, text_new) and np.array_equal(ver_old, ver_new)
    b.check_text(text_old, "the old call")


def test_flat_one_shot_is_the_piecewise_text(hasher):
    """The flat one-shot text against the text update_encode builds from three
    pieces per chunk on flat encoder states."""
    b = sizes_batch("flat")
    one_shot = run(hasher, b, "batch")
    n = b.n
    enc, sha = new_b64_enc_states(n, "flat"), new_states(n)
    text = np.full(b.want.size, FILL, dtype=np.uint8)
    caps = np.array(b.lens, dtype=np.uint32)
    cuts = [(s // 3, s // 3 + (s - s // 3) // 2) for s in b.sizes.tolist()]
    for r in range(3):
        lo = np.array([(0, c[0], c[1])[r] for c in cuts], dtype=np.uint64)
        hi = np.array([(c[0], c[1], s)[r] for c, s in zip(cuts, b.sizes.tolist())], dtype=np.uint64)
        out = hasher.update_encode(enc, sha, b.data, b.offs + lo, (hi - lo).astype(np.uint32), text, b.toffs, caps,
                                   final=np.full(n, r == 2), expected=b.expected)
    _, _, tsizes, ver = out
    assert np.array_equal(tsizes, caps) and np.array_equal(ver, b.verdicts.astype(bool))
    assert np.array_equal(text, one_shot)


def test_flat_text_decodes_back_through_the_flat_pass(hasher):
    """verify_b64 with the flat path on takes the one-shot flat text back to the
    bytes, and its flat pass counts every chunk of more than 54 bytes."""
    b = sizes_batch("flat")
    text = run(hasher, b, "batch")
    out = np.full(b.data.size, FILL, dtype=np.uint8)
    before = H.set_b64_flat(True)
    try:
        stats0 = hasher.b64_flat_stats()
        ver, sizes = hasher.verify_b64(text, b.toffs, np.array(b.lens, dtype=np.uint32), b.sizes, b.digests, out=out,
                                       out_offsets=b.offs)
        stats1 = hasher.b64_flat_stats()
    finally:
        H.set_b64_flat(before)
    assert ver.all() and np.array_equal(sizes, b.sizes)
    for o, c in zip(b.offs.tolist(), b.chunks):
        assert out[o:o + len(c)].tobytes() == c
    assert stats1["flat_chunks"] - stats0["flat_chunks"] == int((b.sizes > 54).sum())

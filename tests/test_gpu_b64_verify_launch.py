"""lbf_b64_verify_launch on the GPU: chunk text resident in device memory
decoded and verified one-shot (bitflood_amd/csrc/b64_verify_launch.hip).

Two yardsticks, neither a path of the launch itself: tests/wire_layouts.py
(`decode`, pinned to xmlrpc++'s recorded answers) with hashlib, and
ChunkHasher.verify_b64 (lbf_b64_verify_batch, which runs the old one-shot
kernels) on the same texts with lbf_set_b64_flat on and off.  Every call is
checked whole: every byte of the output arena -- 0xEE wherever no slot lies,
zeros behind a short decode -- d_out_sizes, verdicts, digests, and `over` and
`redo` read back from d_work.  `redo` must be 0 for every text a tile body can
take, or the scan fallback could hide a broken tile route.

A note on redo and the corpora: the "one-pass" half of disagree_corpus() is
text in the encoder's layout whose decoded length differs from the slot; the
tile body takes it (that is the corpus's point) and reports the length, so its
redo is 0.  The "general" half and every text of scan_corpus() are 1.
"""
import ctypes
import functools
import hashlib

import numpy as np
import pytest

from bitflood_amd import DeviceBuffer, _capi
from bitflood_amd import hashing as H
from tests import wire_flat_model as F
from tests import wire_layouts as W

pytestmark = pytest.mark.gpu

FILL = 0xEE
UINT32_MAX = 0xFFFFFFFF
T, G = W.DEC_BYTES, W.DEC_BYTES * W.DEC_TILES_PER_GROUP
# the flat/canon boundary, one tile, and one, two and more than two workgroups of 4 tiles
SIZES = (0, 1, 2, 3, 53, 54, 55, T - 1, T, T + 1, G - 1, G, G + 1, 2 * G + 1)
assert SIZES == (0, 1, 2, 3, 53, 54, 55, 3887, 3888, 3889, 15551, 15552, 15553, 31105)
EMPTY_SHA = hashlib.sha1(b"").digest()


class Entry:
    """One chunk of a call: its text, its slot's size, the digest the receiver
    expects, where text and slot start mod 16 (None: wherever the gaps put
    them), and whether the call's bounds leave it out."""
    __slots__ = ("text", "cap", "exp", "tphase", "sphase", "desc", "out_of_bounds")

    def __init__(self, text, cap, exp, desc, tphase=None, sphase=None, out_of_bounds=False):
        self.text, self.cap, self.exp, self.desc = bytes(text), int(cap), bytes(exp), desc
        self.tphase, self.sphase, self.out_of_bounds = tphase, sphase, out_of_bounds


def entry_of(data, layout, desc="", **kw):
    text = W.xmlrpc_text(data) if layout == "xmlrpc" else F.text(data)
    return Entry(text, len(data), hashlib.sha1(data).digest(), f"{len(data)} B {layout} {desc}", **kw)


def from_corpus(c):
    return [Entry(t, cap, hashlib.sha1(d).digest() if ok else bytes(20), desc, tphase=tp, sphase=sp)
            for t, d, cap, desc, tp, sp, ok in zip(c.texts, c.chunks, c.caps, c.desc, c.tphase, c.sphase, c.digest_ok)]


def want_redo(e):
    """Whether the tile pass hands the chunk to the scan: the route by the
    chunk's own lengths, then that route's layout."""
    if F.is_candidate(len(e.text), e.cap):
        return not F.is_flat(e.text)
    return not W.is_encoder_layout(e.text)


class Expect:
    """What one entry must give, from `decode` and hashlib alone."""
    __slots__ = ("slot", "size", "over", "verdict", "digest", "redo")

    def __init__(self, e):
        if e.out_of_bounds:
            self.slot, self.size, self.over, self.verdict = None, UINT32_MAX, 0, 0
            self.digest, self.redo = EMPTY_SHA, 0
            return
        w = W.decode(e.text)
        kept = w[:e.cap]
        self.slot = kept + bytes(e.cap - len(kept))
        self.over = 1 if len(w) > e.cap else 0
        self.size = e.cap + 1 if self.over else len(w)
        self.verdict = 1 if (len(w) == e.cap and hashlib.sha1(w).digest() == e.exp) else 0
        self.digest = hashlib.sha1(kept).digest()
        self.redo = 1 if want_redo(e) else 0


class Laid:
    """The entries laid out in two 0xEE-filled arenas, in caller order, with
    gaps between texts and between slots, and the call's tables."""

    def __init__(self, entries):
        self.entries = entries
        n = self.n = len(entries)
        self.toff, self.ooff = np.zeros(n, np.uint64), np.zeros(n, np.uint64)
        self.tlen = np.array([len(e.text) for e in entries], np.uint32)
        self.caps = np.array([e.cap for e in entries], np.uint32)
        self.exp = np.frombuffer(b"".join(e.exp for e in entries), np.uint8).reshape(n, 20).copy()
        tcur = ocur = 0
        for i, e in enumerate(entries):
            self.toff[i] = tcur = self._place(tcur, e.tphase)
            self.ooff[i] = ocur = self._place(ocur, e.sphase)
            tcur += len(e.text)
            ocur += e.cap
        self.text = np.full(tcur + 48, FILL, np.uint8)
        for i, e in enumerate(entries):
            self.text[int(self.toff[i]):int(self.toff[i]) + len(e.text)] = np.frombuffer(e.text, np.uint8)
        self.out_bytes = ocur + 48

    @staticmethod
    def _place(cur, phase):
        p = cur + 3  # never touching the entry in front
        if phase is not None:
            p += (phase - p) % 16
        return p


class Device:
    """A Laid call's arenas and tables in device memory (hipMalloc is
    256-byte aligned: an offset's phase mod 16 is the address's)."""

    def __init__(self, laid):
        n = max(laid.n, 1)
        self.laid = laid
        self.bufs = {}
        for name, host in (("text", laid.text), ("toff", laid.toff), ("tlen", laid.tlen), ("caps", laid.caps),
                           ("ooff", laid.ooff), ("exp", laid.exp)):
            self.bufs[name] = DeviceBuffer(max(host.nbytes, 16))
            if host.nbytes:
                self.bufs[name].upload(host)
        for name, nbytes in (("out", laid.out_bytes), ("sizes", 4 * n), ("dig", 20 * n), ("ver", n), ("work", 2 * n)):
            self.bufs[name] = DeviceBuffer(max(nbytes, 16))

    def __enter__(self):
        return self

    def __exit__(self, *a):
        for b in self.bufs.values():
            b.free()

    def launch(self, max_text_len=None, max_size=None, digests=True, verdicts=True, stream=None, suffix=""):
        """Fill the results with 0xEE, enqueue one call.  `suffix` names a
        second set of result buffers (two streams)."""
        L, b = self.laid, self.bufs
        for name in ("out", "sizes", "dig", "ver", "work"):
            if name + suffix not in b:
                b[name + suffix] = DeviceBuffer(b[name].nbytes)
            b[name + suffix].upload(np.full(b[name].nbytes, FILL, np.uint8))
        H.verify_b64_launch(b["text"], b["toff"], b["tlen"], L.n,
                            int(L.tlen.max(initial=0)) if max_text_len is None else max_text_len, b["caps"],
                            int(L.caps.max(initial=0)) if max_size is None else max_size, b["out" + suffix], b["ooff"],
                            b["sizes" + suffix], b["work" + suffix], digests=b["dig" + suffix] if digests else None,
                            expected=b["exp"] if verdicts else None, verdicts=b["ver" + suffix] if verdicts else None,
                            stream=stream)

    def results(self, suffix=""):
        L, b, n = self.laid, self.bufs, self.laid.n
        work = b["work" + suffix].download(2 * n)
        return dict(out=b["out" + suffix].download(L.out_bytes), sizes=b["sizes" + suffix].download(4 * n, dtype=np.uint32),
                    dig=b["dig" + suffix].download(20 * n).reshape(n, 20), ver=b["ver" + suffix].download(n),
                    over=work[:n], redo=work[n:])


def check(laid, expects, res, digests=True, verdicts=True):
    """Every result of one call against `expects`; every arena byte outside the slots."""
    out = res["out"]
    mask = np.ones(out.size, bool)
    for i, (e, x) in enumerate(zip(laid.entries, expects)):
        o = int(laid.ooff[i])
        got = out[o:o + e.cap].tobytes()
        if x.slot is None:
            assert got == bytes([FILL]) * e.cap, ("slot of a chunk over a bound touched", e.desc)
        else:
            assert got == x.slot, (e.desc, "bytes", _first_diff(got, x.slot))
            mask[o:o + e.cap] = False
        assert int(res["sizes"][i]) == x.size, (e.desc, "size", int(res["sizes"][i]), x.size)
        assert int(res["over"][i]) == x.over, (e.desc, "over")
        assert int(res["redo"][i]) == x.redo, (e.desc, "redo", int(res["redo"][i]), x.redo)
        if verdicts:
            assert int(res["ver"][i]) == x.verdict, (e.desc, "verdict", int(res["ver"][i]), x.verdict)
        if digests:
            assert res["dig"][i].tobytes() == x.digest, (e.desc, "digest")
    assert (out[mask] == FILL).all(), ("bytes outside the slots written", np.flatnonzero(out[mask] != FILL)[:8])
    if not verdicts:
        assert (res["ver"] == FILL).all()
    if not digests:
        assert (res["dig"] == FILL).all()


def _first_diff(a, b):
    k = next((k for k in range(min(len(a), len(b))) if a[k] != b[k]), min(len(a), len(b)))
    return f"first difference at byte {k} of {len(b)}"


def check_against_batch(hasher, laid, res):
    """lbf_b64_verify_batch on the same texts, the flat path on and off: the
    same bytes, out_sizes and verdicts."""
    for flat in (True, False):
        before = H.set_b64_flat(flat)
        try:
            out = np.full(laid.out_bytes, FILL, np.uint8)
            ver, sizes = hasher.verify_b64(laid.text, laid.toff, laid.tlen, laid.caps, laid.exp, out=out,
                                           out_offsets=laid.ooff)
        finally:
            H.set_b64_flat(before)
        assert np.array_equal(out, res["out"]), ("bytes differ from lbf_b64_verify_batch", flat)
        assert np.array_equal(sizes, res["sizes"]), ("sizes differ from lbf_b64_verify_batch", flat)
        assert np.array_equal(ver, res["ver"].astype(bool)), ("verdicts differ from lbf_b64_verify_batch", flat)


def run(hasher, entries, against_batch=True):
    """One call over `entries`, checked whole against both yardsticks."""
    laid, expects = Laid(entries), [Expect(e) for e in entries]
    with Device(laid) as dev:
        dev.launch()
        H.synchronize()
        res = dev.results()
    check(laid, expects, res)
    if against_batch:
        check_against_batch(hasher, laid, res)
    return expects, res


# ------------------------------------------------------------------ 1. sizes
@functools.lru_cache(maxsize=None)
def size_entries():
    """Every size in both layouts at every phase mod 16 of text and slot, the
    layouts alternating in caller order."""
    out = []
    for k, n in enumerate(SIZES):
        d = W.chunk_bytes(n, seed=11)
        for p in range(16):
            for layout in (("xmlrpc", "flat") if (k + p) % 2 else ("flat", "xmlrpc")):
                out.append(entry_of(d, layout, f"text%16={p} slot%16={(7 * p + 5) % 16}", tphase=p,
                                    sphase=(7 * p + 5) % 16))
    return out


def test_sizes_in_both_layouts_at_every_phase(hasher):
    entries = size_entries()
    assert len(entries) == 2 * 16 * len(SIZES)
    assert {e.sphase for e in entries} == set(range(16)) == {e.tphase for e in entries}
    expects, res = run(hasher, entries)
    # undamaged text of either layout stays on its tile route, and every chunk verifies
    assert not res["redo"].any() and not res["over"].any() and res["ver"].all()
    flat_routed = sum(F.is_candidate(len(e.text), e.cap) for e in entries)
    assert flat_routed == 16 * sum(n > 54 and F.flat_len(n) != W.b64_len(n) for n in SIZES) > 0


def test_short_and_long_decodes_and_a_wrong_digest(hasher):
    """Texts that decode to less and to more than the slot, in both layouts,
    at one tile and past a workgroup: zeros behind the short decode, cap + 1
    for the long one; and a chunk of the right length with a wrong digest."""
    entries = []
    for n in (55, T, G + 1):
        d = W.chunk_bytes(n + 40, seed=12)
        for layout, text in (("xmlrpc", W.xmlrpc_text), ("flat", F.text)):
            for L in (n - 40, n - 1, n + 1, n + 40):
                entries.append(Entry(text(d[:L]), n, hashlib.sha1(d[:n]).digest(), f"{layout} L={L} cap={n}",
                                     sphase=L % 16))
            entries.append(Entry(text(d[:n]), n, hashlib.sha1(d[:n - 1]).digest(), f"{layout} wrong digest"))
            entries.append(entry_of(d[:n], layout, "right"))
    expects, res = run(hasher, entries)
    assert res["ver"].sum() == 6 and res["over"].sum() == 12
    assert sum(x.size < e.cap for e, x in zip(entries, expects)) == 12


# ----------------------------------------------------------------- 2. routes
@functools.lru_cache(maxsize=None)
def disagree_entries():
    return from_corpus(W.disagree_corpus())


@functools.lru_cache(maxsize=None)
def scan_entries():
    return from_corpus(W.scan_corpus())


def test_routes_of_the_disagree_corpus(hasher):
    entries = disagree_entries()
    expects, res = run(hasher, entries)
    general = np.array(["general" in e.desc for e in entries])
    assert general.sum() == len(entries) // 2
    assert (res["redo"][general] == 1).all() and (res["redo"][~general] == 0).all()
    assert res["over"].any() and not res["ver"].any()  # no pair has L == C


def test_routes_of_the_scan_corpus(hasher):
    entries = scan_entries()
    expects, res = run(hasher, entries)
    assert (res["redo"] == 1).all()
    assert res["over"].any() and res["ver"].any()


# ----------------------------------------------------------------- 3. damage
def _flat_edge_positions(text_len):
    """edge_positions for unbroken text: 80 characters to both sides of the
    first tile edge, of the workgroup edge and of a later tile edge, 17 around
    scan trips 1, 2 and 6, the last 80."""
    ps = set()
    for tile in (1, W.DEC_TILES_PER_GROUP, 5):
        ps.update(range(tile * F.TILE_TEXT - 80, tile * F.TILE_TEXT + 80))
    for k in (1, 2, 6):
        ps.update(range(W.SCAN_CHARS * k - 17, W.SCAN_CHARS * k + 18))
    ps.update(range(text_len - 80, text_len))
    return sorted(p for p in ps if 0 <= p < text_len)


def _flat_damaged(sizes, kind, places, name):
    out = []
    for n in sizes:
        d = W.chunk_bytes(n)
        t = F.text(d)
        out.append(entry_of(d, "flat", f"{name} undamaged"))
        ps = places(len(t))
        if kind == "cut" or kind.startswith("ins_"):
            ps = list(ps) + [len(t)]
        for p in ps:
            out.append(Entry(W.damage(t, kind, p), n, hashlib.sha1(d).digest(), f"{name} flat {n} B {kind} at {p}",
                             tphase=p % 16, sphase=(p // 16) % 16))
    return out


PERIOD_STEP = 5  # every fifth position of the 16-line period, the offset rotating with the kind


@pytest.mark.parametrize("kind", W.KINDS)
def test_damage_at_the_edges_in_both_layouts(hasher, kind):
    entries = from_corpus(W.edge_corpus(kind)) + _flat_damaged(W.EDGE_SIZES, kind, _flat_edge_positions, "edges")
    expects, res = run(hasher, entries)
    assert (res["redo"] == 1).any() and (res["redo"] == 0).any() and res["ver"].any()


@pytest.mark.parametrize("kind", W.KINDS)
def test_damage_over_a_period_in_both_layouts(hasher, kind):
    entries = from_corpus(W.period_corpus(kind, step=PERIOD_STEP))
    first = W.KINDS.index(kind) % PERIOD_STEP
    entries += _flat_damaged(W.PERIOD_SIZES, kind, lambda n: range(first, n, PERIOD_STEP), "period")
    expects, res = run(hasher, entries)
    assert (res["redo"] == 1).any() and res["ver"].any()


# ----------------------------------------------------------------- 4. bounds
def test_chunks_over_a_bound_are_left_alone(hasher):
    """One chunk's text is longer than max_text_len, another's size larger than
    max_size: UINT32_MAX, verdict 0, slot untouched; their neighbours as ever."""
    # a slot no larger than its neighbours', a text (padded with separators) longer than max_text_len
    d = W.chunk_bytes(2400, seed=21)
    big_text = Entry(W.xmlrpc_text(d) + b" " * 600, 2400, hashlib.sha1(d).digest(), "text over max_text_len",
                     out_of_bounds=True)
    # a text no longer than its neighbours', a slot larger than max_size
    big_slot = Entry(W.xmlrpc_text(W.chunk_bytes(100, seed=22)), 2600, bytes(20), "size over max_size",
                     out_of_bounds=True)
    around = [entry_of(W.chunk_bytes(n, seed=23), layout, "neighbour") for n, layout in
              ((2500, "xmlrpc"), (2500, "flat"), (55, "flat"), (0, "xmlrpc"), (2499, "xmlrpc"))]
    entries = [around[0], big_text, around[1], around[2], big_slot, around[3], around[4]]
    max_text_len = max(len(e.text) for e in around)
    assert len(big_text.text) > max_text_len >= len(big_slot.text) and big_slot.cap > 2500 >= big_text.cap
    laid, expects = Laid(entries), [Expect(e) for e in entries]
    with Device(laid) as dev:
        dev.launch(max_text_len=max_text_len, max_size=2500)
        H.synchronize()
        res = dev.results()
    check(laid, expects, res)
    assert list(res["sizes"][[1, 4]]) == [UINT32_MAX, UINT32_MAX] and list(res["ver"]) == [1, 0, 1, 1, 0, 1, 1]


# ---------------------------------------------------- 5. more than one grid
@functools.lru_cache(maxsize=None)
def many_entries():
    """65,537 chunks cross the 65,535-chunk split: 3 bytes each, and every
    997th (and the three around the split) 55 bytes of unbroken text."""
    n = W.CHUNKS_PER_LAUNCH + 2
    stream = W.chunk_bytes(3 * n + 64, seed=31)
    out = []
    for i in range(n):
        if i % 997 == 5 or i in (n - 3, n - 2, n - 1):
            out.append(entry_of(stream[3 * i:3 * i + 55], "flat", f"chunk {i}"))
        else:
            out.append(entry_of(stream[3 * i:3 * i + 3], "xmlrpc", f"chunk {i}"))
    return out


def test_more_chunks_than_one_grid(hasher):
    entries = many_entries()
    assert len(entries) == 65537
    expects, res = run(hasher, entries)
    assert res["ver"].all() and not res["redo"].any()
    assert sum(F.is_candidate(len(e.text), e.cap) for e in entries) >= 66


def test_slices_corpus(hasher):
    """One launch slice and 300 more chunks of 0..60 bytes, every 7th with a
    junk character, every 11th with a wrong expected digest."""
    expects, res = run(hasher, from_corpus(W.slices_corpus()))
    assert res["redo"].sum() >= len(expects) // 8 and 0 < res["ver"].sum() < len(expects)


# ------------------------------------------------------ 6. null combinations
@pytest.mark.parametrize("digests,verdicts", [(True, False), (False, True), (False, False)],
                         ids=["digests-only", "verdicts-only", "decode-only"])
def test_null_combinations(hasher, digests, verdicts):
    entries = size_entries()[::3] + disagree_entries()[::5] + scan_entries()[::4]
    laid, expects = Laid(entries), [Expect(e) for e in entries]
    with Device(laid) as dev:
        dev.launch(digests=digests, verdicts=verdicts)
        H.synchronize()
        res = dev.results()
    check(laid, expects, res, digests=digests, verdicts=verdicts)


# ---------------------------------------------------------------- 7. streams
def test_two_streams_with_separate_work(hasher):
    """The same call enqueued on two streams at once, each with its own
    outputs and d_work, gives what one call gives."""
    entries = size_entries()[1::2] + scan_entries()[::3]
    laid, expects = Laid(entries), [Expect(e) for e in entries]
    lib = _capi.load()
    streams = [ctypes.c_void_p(), ctypes.c_void_p()]
    for st in streams:
        _capi.check(lib.lbf_stream_create(ctypes.byref(st)))
    try:
        with Device(laid) as dev:
            dev.launch(stream=streams[0])
            dev.launch(stream=streams[1], suffix="2")
            for st in streams:
                _capi.check(lib.lbf_stream_synchronize(st))
            one, two = dev.results(), dev.results("2")
            dev.launch()  # and on the default stream
            H.synchronize()
            alone = dev.results()
    finally:
        for st in streams:
            _capi.check(lib.lbf_stream_destroy(st))
    for res in (one, two, alone):
        check(laid, expects, res)
    for k in one:
        assert np.array_equal(one[k], two[k]) and np.array_equal(one[k], alone[k]), k

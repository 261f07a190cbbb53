"""The device launch paths past byte 2^32 of their buffers and past 65,536
entries in one launch (lbf_sha1_launch, lbf_sha1_uniform_launch,
lbf_sha1_update_launch, lbf_b64_update_launch; update_chunks and update_text
over host arrays larger than 4 GiB).

The layouts come from tests/large_index.py, and tests/test_large_index.py shows
on the CPU what they reach: entries below, across, exactly at and above byte
2^32 of one allocation whose positions mod 2^32 hold other bytes (reads) or the
fill value (writes), so that an address kept in 32 bits gives a wrong answer
inside the allocation and never a fault; and entry counts of the launchers'
threshold + 64 + 37, read from the sources.  Only the windows of a large buffer
that hold data are ever uploaded or read back.

Expected values come from oracle.sha1_batch, hashlib, tests/sha1_model.py and
the wire models (tests/wire_layouts.py, tests/wire_piece_model.py), never from a
GPU path.  Outputs are pre-filled with 0xA5 or 0xEE; written windows are
compared byte for byte, alias windows and guard entries for their fill.
"""
import functools
import os
import re

import numpy as np
import pytest

from bitflood_amd import B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import large_index as L
from tests import wire_layouts as W
from tests import wire_piece_model as M
from tests.test_gpu_b64_fused import LAYOUTS, SIZES, TILE_TEXT, big_text
from tests.test_gpu_b64_update import Chain, model_update
from tests.test_gpu_device_paths import FILL, VARIANTS, Device, _assert_rows, _flip_expected, _rows, _verdict_pattern
from tests.test_gpu_update import FIRST, SECOND, _raw_update, digests_of, sha1

pytestmark = pytest.mark.gpu

LINE = L.LINE
EE = 0xEE
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {0: "auto", 1: "lane", 7: "pc4b64", 10: "pcx5", 11: "lds2", 12: "pc4x2"}


@pytest.fixture(params=[0] + VARIANTS, ids=lambda v: NAMES[v])
def variant(request):
    H.set_kernel_variant(request.param)
    yield request.param
    H.set_kernel_variant(0)


@pytest.fixture(params=VARIANTS, ids=lambda v: NAMES[v])
def forced(request):
    H.set_kernel_variant(request.param)
    yield request.param
    H.set_kernel_variant(0)


def _large():
    buf = DeviceBuffer(LINE + (1 << 20))
    try:
        yield buf
    finally:
        buf.free()


@pytest.fixture(scope="module")
def big():
    """4 GiB + 1 MiB of device memory for sources and text (read)."""
    yield from _large()


@pytest.fixture(scope="module")
def big2():
    """The same again for slots and records (written)."""
    yield from _large()


def _anchor(sizes):
    """The entry of more than 64 bytes nearest the middle: the one laid at or across the line."""
    mid = len(sizes) // 2
    return min((k for k in range(len(sizes)) if sizes[k] > 64), key=lambda k: (abs(k - mid), k))


def _upload(buf, ranges):
    assert ranges.alloc <= buf.nbytes
    for offset, data in ranges.uploads():
        buf.upload(data, offset)


def _frozen(a):
    a.setflags(write=False)
    return a


def _describe(r, kinds, skip=0, what=""):
    """Names entry i of a launch that starts at entry `skip` of the ranges r."""
    def describe(i):
        i = int(i)
        return (f"entry {i} ({kinds[skip + i]}): offset 2^32{int(r.offsets[skip + i]) - LINE:+d} size "
                f"{int(r.sizes[skip + i])}, lane {i % 64} of wave {i // 64} {what}")
    return describe


def _pick(kinds, kind, k=0):
    return [i for i, x in enumerate(kinds) if x == kind][k]


# ------------------------------------------------------------ a. the table form past the line
@pytest.fixture(scope="module")
def table(oracle):
    r = L.table_case()
    return r, _frozen(oracle.sha1_batch(r.window, r.rel(), r.sizes, nthreads=8))


def test_table_entries_past_the_line(variant, table, big):
    """lbf_sha1_launch with offsets below, across, at and above 2^32, shuffled:
    hash mode, then verify mode with one expected digest off by a bit on each
    side of the line and one across it."""
    r, want = table
    n, kinds = r.n, r.kinds()
    describe = _describe(r, kinds)
    _upload(big, r)
    flips = [_pick(kinds, L.BELOW, 3), _pick(kinds, L.STRADDLE, 1), _pick(kinds, L.ABOVE, 5)]
    exp = _flip_expected(want.copy(), flips)
    with Device() as dev:
        d_off, d_size = dev.put(r.offsets), dev.put(r.sizes)
        d_out = dev.filled(20 * (n + 8))
        H.batch_launch(big, d_off, d_size, n, d_out)
        H.synchronize()
        _assert_rows(_rows(d_out, n), want, describe, "lbf_sha1_launch")
        assert (d_out.download(160, 20 * n) == FILL).all()
        d_exp, d_ver = dev.put(exp), dev.filled(n + 8)
        H.batch_launch(big, d_off, d_size, n, None, expected=d_exp, verdicts=d_ver)
        H.synchronize()
        _assert_rows(d_ver.download(n), _verdict_pattern(n, flips), describe, "lbf_sha1_launch verdicts")
        assert (d_ver.download(8, n) == FILL).all()


# ------------------------------------------------------------ b. the uniform form past the line
@pytest.fixture(scope="module")
def uniform(oracle):
    out = []
    for case in L.uniform_cases():
        r = L.uniform_ranges(*case)
        out.append((case, r, _frozen(oracle.sha1_batch(r.window, r.rel(), r.sizes, nthreads=8))))
    return out


def test_uniform_chunks_past_the_line(variant, uniform, big):
    """lbf_sha1_uniform_launch over chunks on both sides of byte 2^32 of the
    region, one across it (odd chunk size) or one exactly at it (a chunk size
    that divides 2^32), from first_chunk and from one chunk later; hash mode and
    verify mode."""
    for (cs, first, n, length), r, want in uniform:
        kinds = r.kinds()
        _upload(big, r)
        with Device() as dev:
            for skip in (0, 1):
                m = n - skip
                describe = _describe(r, kinds, skip, f"chunk size {cs}, from chunk {first + skip}")
                across = _pick(kinds, L.STRADDLE if L.STRADDLE in kinds else L.AT) - skip
                flips = [1, across, m - 1]
                exp = _flip_expected(want[skip:].copy(), flips)
                d_dig, d_exp, d_ver = dev.filled(20 * (m + 8)), dev.put(exp), dev.filled(m + 8)
                H.uniform_launch(big, length, cs, first + skip, m, d_dig, d_exp, d_ver)
                H.synchronize()
                _assert_rows(_rows(d_dig, m), want[skip:], describe, f"uniform launch from chunk {first + skip}")
                _assert_rows(d_ver.download(m), _verdict_pattern(m, flips), describe, "uniform launch verdicts")
                assert (d_dig.download(160, 20 * m) == FILL).all() and (d_ver.download(8, m) == FILL).all()


# ------------------------------------------------------------ c. resumable SHA-1: pieces past the line
def _mid_records(prefixes):
    return M.sha_records([M.sha_state(p, len(p)) for p in prefixes], STATE_DTYPE)


def test_update_pieces_past_the_line(big):
    """lbf_sha1_update_launch: every chain fed in two launches from offsets
    around byte 2^32 at the source phases 0, 1, 8 and 15, the first launch's
    pieces around one that starts at 2^32, the second's around one across it;
    the final flags come with the second."""
    combos = L.thinned(FIRST, SECOND)
    n = len(combos)
    first, second = L.piece_cases([a for a, _ in combos], [b for _, b in combos])
    _upload(big, first)  # one window for both launches
    p1 = [first.true_bytes(k) for k in range(n)]
    p2 = [second.true_bytes(k) for k in range(n)]
    want = digests_of(a + b for a, b in zip(p1, p2))
    with Device() as dev:
        d_states = dev.put(new_states(n))
        d_off, d_size = dev.put(first.offsets), dev.put(first.sizes)
        H.update_launch(d_states, n, None, big, d_off, d_size, None, n, None)
        H.synchronize()
        mid = d_states.download(96 * n).view(STATE_DTYPE)
        bad = M.sha_records_differ(mid, _mid_records(p1))
        assert not bad, [(k, combos[k], first.kinds()[k], mid[k]) for k in bad[:3]]
        d_off2, d_size2 = dev.put(second.offsets), dev.put(second.sizes)
        d_fin, d_dig = dev.put(np.ones(n, dtype=np.uint8)), dev.filled(20 * (n + 4))
        H.update_launch(d_states, n, None, big, d_off2, d_size2, d_fin, n, d_dig)
        H.synchronize()
        kinds = list(zip(first.kinds(), second.kinds()))
        _assert_rows(_rows(d_dig, n), want, lambda i: f"chain {int(i)} {combos[int(i)]} {kinds[int(i)]}", "digests")
        assert (d_dig.download(80, 20 * n) == FILL).all()
        assert d_states.download(96 * n).tobytes() == new_states(n).tobytes()


# ------------------------------------------------------------ d. resumable SHA-1: records past the line
def test_update_records_past_the_line(big2):
    """lbf_sha1_update_launch on a state array of 2^32 / 96 + 64 records: the
    records below, across and above byte 2^32 of the array, named through
    state_of in shuffled order, go mid-chunk and then fresh; the bytes at the
    same positions minus 2^32 and every other record of the window keep their
    0xEE."""
    rng = np.random.default_rng(96)
    named = np.array(L.STATE_INDICES, dtype=np.uint32)[rng.permutation(len(L.STATE_INDICES))]
    n, n_states = named.size, L.N_STATES
    assert 96 * n_states <= big2.nbytes
    w0 = min(L.STATE_INDICES) - 1                         # the window of records read back
    window = np.full((n_states - w0, 96), EE, dtype=np.uint8)
    for s in L.STATE_INDICES:
        window[s - w0] = new_states(1).view(np.uint8)
    alias = np.full(96 * n_states - LINE, EE, dtype=np.uint8)
    big2.upload(alias, 0)
    big2.upload(window, 96 * w0)
    sizes1, sizes2 = [63, 1, 64, 200, 0][:n], [130, 55, 0, 56, 9][:n]
    data = rng.integers(0, 256, sum(sizes1) + sum(sizes2) + 1, dtype=np.uint8)
    cuts = np.cumsum([0] + sizes1 + sizes2)
    p1 = [data[cuts[k]:cuts[k + 1]].tobytes() for k in range(n)]
    p2 = [data[cuts[n + k]:cuts[n + k + 1]].tobytes() for k in range(n)]

    def check_window(records, what):
        got = big2.download(window.size, 96 * w0).reshape(-1, 96)
        want = window.copy()
        for k, s in enumerate(named):
            want[int(s) - w0] = records[k:k + 1].view(np.uint8)
        others = np.setdiff1d(np.arange(n_states - w0), named.astype(np.int64) - w0)
        assert (got[others] == EE).all(), (what, "a record no piece names was written", L.STATE_NEIGHBOUR)
        bad = M.sha_records_differ(got.reshape(-1).view(STATE_DTYPE)[named.astype(np.int64) - w0], records)
        assert not bad, (what, [(int(named[k]) - L.S, got[int(named[k]) - w0]) for k in bad])
        assert (big2.download(alias.size, 0) == EE).all(), (what, "bytes at the records' positions mod 2^32 written")

    with Device() as dev:
        d_so, d_data = dev.put(named), dev.put(data)
        d_off, d_size = dev.put(cuts[:n].astype(np.uint64)), dev.put(np.array(sizes1, dtype=np.uint32))
        H.update_launch(big2, n_states, d_so, d_data, d_off, d_size, None, n, None)
        H.synchronize()
        check_window(_mid_records(p1), "first launch")
        d_off2, d_size2 = dev.put(cuts[n:2 * n].astype(np.uint64)), dev.put(np.array(sizes2, dtype=np.uint32))
        d_fin, d_dig = dev.put(np.ones(n, dtype=np.uint8)), dev.filled(20 * (n + 2))
        H.update_launch(big2, n_states, d_so, d_data, d_off2, d_size2, d_fin, n, d_dig)
        H.synchronize()
        dig = d_dig.download(20 * (n + 2)).reshape(-1, 20)
        assert np.array_equal(dig[:n], digests_of(a + b for a, b in zip(p1, p2))), [int(s) - L.S for s in named]
        assert (dig[n:] == FILL).all()
        check_window(new_states(n), "second launch")


# ------------------------------------------------------------ e. base64 text and slots past the line
@functools.lru_cache(maxsize=None)
def _text_chains():
    """25 chains: both layouts' five-tile texts cut in three around the first
    tile edge, a few texts below one tile, one with a character replaced by junk
    (verdict 0), one whose slot is short (verdict 0), one with junk inserted
    (skipped: verdict 1)."""
    chains = []
    for layout in LAYOUTS:
        d, t = big_text(layout, seed=1)
        tile = TILE_TEXT[layout]
        chains += [Chain([t[:a], t[a:a + tile + e], t[a + tile + e:]], chunk=d, desc=f"{layout} cuts at {a}, {e}")
                   for a, e in ((0, 0), (1, -12), (2, 7), (3, -1), (37, 12), (37, 1), (2, -5), (1, 0))]
    for k, size in enumerate(SIZES[2:]):
        d = W.chunk_bytes(size)
        t = W.xmlrpc_text(d)
        chains.append(Chain([t[:k], t[k:len(t) // 2], t[len(t) // 2:]], chunk=d, desc=f"{size} B"))
    d, t = big_text("xmlrpc", seed=2)
    hurt = W.damage(t, "junk", 9000)
    chains.append(Chain([hurt[:5000], hurt[5000:12000], hurt[12000:]], cap=len(d), chunk=d, desc="character replaced"))
    chains.append(Chain([t[:100], t[100:20000], t[20000:]], cap=len(d) - 5, desc="slot 5 bytes short"))
    assert not chains[-2].verdict and not chains[-1].verdict and chains[-1].size == len(d) - 4
    junk = W.damage(t, "ins_junk", 9001)  # skipped by the decoder: the bytes and the verdict stay right
    chains.append(Chain([junk[:70], junk[70:9002], junk[9002:]], cap=len(d), chunk=d, desc="junk inserted"))
    assert chains[-1].verdict and chains[-1].want == d
    assert sum(c.verdict for c in chains) == len(chains) - 2 and len(chains) == 25
    # the slots in an order that puts long ones around the line and short ones on both sides
    order = np.random.default_rng(24).permutation(len(chains))
    return [chains[i] for i in order]


class WindowFeed:
    """tests/test_gpu_b64_update.py's DeviceFeed with `out` and `text` of more
    than 4 GiB each: the slots lie around byte 2^32 of `out` (tests/large_index
    slot_case), each round's pieces around byte 2^32 of `text` (text_case), and
    only the windows travel."""

    def __init__(self, chains, slot_mode, text_buf, out_buf):
        self.chains, self.text_buf, self.out_buf = chains, text_buf, out_buf
        n = len(chains)
        caps = [c.cap for c in chains]
        anchor = _anchor(caps)
        self.slot_mode = slot_mode
        self.slots = L.slot_case(caps, anchor, slot_mode, EE)
        assert self.slots.kinds()[anchor] == slot_mode
        self.want = self.slots.window.copy()
        self.model, self.sofar = [M.init()] * n, [b""] * n
        self.expected = np.frombuffer(b"".join(c.expected for c in chains), dtype=np.uint8).reshape(n, 20)
        self.rounds = max(len(c.pieces) for c in chains)
        _upload(out_buf, self.slots)
        self.dev = Device()
        self.d_b64, self.d_sha = self.dev.put(new_b64_states(n)), self.dev.put(new_states(n))

    def close(self):
        self.dev.__exit__()

    def run_round(self, r):
        ch, n = self.chains, len(self.chains)
        live = [k for k, c in enumerate(ch) if r < len(c.pieces)]
        m = len(live)
        fin = np.array([r == len(ch[k].pieces) - 1 for k in live], dtype=np.uint8)
        lens = [len(ch[k].pieces[r]) for k in live]
        mode = (L.AT, L.STRADDLE)[(r + (self.slot_mode == L.AT)) % 2]
        anchor = _anchor(lens)
        t = L.text_case(lens, anchor, mode, phase=(9, 0, 3)[r % 3], seed=100 + r)
        assert t.kinds()[anchor] == mode and {L.BELOW, L.ABOVE} <= set(t.kinds())
        for j, k in enumerate(live):
            a = int(t.offsets[j]) - t.lo
            t.window[a:a + lens[j]] = np.frombuffer(ch[k].pieces[r], dtype=np.uint8)
        _upload(self.text_buf, t)
        dev = self.dev
        d_so, d_toff = dev.put(np.array(live, dtype=np.uint32)), dev.put(t.offsets)
        d_tlen, d_fin = dev.put(np.array(lens, dtype=np.uint32)), dev.put(fin)
        d_ooff, d_caps = dev.put(self.slots.offsets[live]), dev.put(self.slots.sizes[live])
        d_osz, d_dig = dev.put(np.full(m, 0xEEEEEEEE, dtype=np.uint32)), dev.put(np.full(20 * m, EE, dtype=np.uint8))
        d_exp, d_ver = dev.put(self.expected[live]), dev.put(np.full(m, EE, dtype=np.uint8))
        d_poff, d_psz = dev.put(np.full(m, EE, dtype=np.uint64)), dev.put(np.full(m, EE, dtype=np.uint32))
        H.b64_update_launch(self.d_b64, self.d_sha, n, d_so, self.text_buf, d_toff, d_tlen, d_fin, m, self.out_buf,
                            d_ooff, d_caps, d_osz, d_dig, d_exp, d_ver, d_poff, d_psz)
        H.synchronize()
        osz, ver = d_osz.download(4 * m, dtype=np.uint32), d_ver.download(m)
        dig = d_dig.download(20 * m).reshape(m, 20)
        lo = self.slots.lo
        for j, k in enumerate(live):
            c = ch[k]
            before = len(self.sofar[k])
            where = f"{c.desc}; slot {self.slots.kinds()[k]}, text {t.kinds()[j]}, round {r}"
            if fin[j]:
                self.model[k], self.sofar[k] = M.init(), c.want
                assert osz[j] == c.size and ver[j] == int(c.verdict), (where, int(osz[j]), c.size, int(ver[j]))
                assert dig[j].tobytes() == sha1(c.want[:c.cap]), where
            else:
                self.model[k], new = model_update(self.model[k], c.pieces[r])
                self.sofar[k] += new
                assert osz[j] == 0xEEEEEEEE and ver[j] == EE and (dig[j] == EE).all(), where
            s, a, b = int(self.slots.offsets[k]) - lo, min(before, c.cap), min(len(self.sofar[k]), c.cap)
            self.want[s + a:s + b] = np.frombuffer(self.sofar[k][a:b], dtype=np.uint8)
        got = self.out_buf.download(self.want.size, lo)
        wrong = np.flatnonzero(got != self.want)
        assert wrong.size == 0, (r, "first wrong byte at 2^32%+d" % (lo + int(wrong[0]) - LINE), self.where(wrong[0]))
        alias = self.out_buf.download(self.slots.alias.size, 0)
        wrong = np.flatnonzero(alias != EE)
        assert wrong.size == 0, (r, f"out written at byte {int(wrong[0])}: a slot position taken mod 2^32")
        b64 = self.d_b64.download(16 * n).view(B64_STATE_DTYPE)
        assert b64.tobytes() == M.b64_records(self.model, B64_STATE_DTYPE).tobytes(), r
        sha = self.d_sha.download(96 * n).view(STATE_DTYPE)
        done = [r >= len(c.pieces) - 1 for c in ch]
        want_sha = M.sha_records([M.sha_state(b"" if done[k] else self.sofar[k], c.cap) for k, c in enumerate(ch)],
                                 STATE_DTYPE)
        bad = M.sha_records_differ(sha, want_sha)
        assert not bad, (r, [(ch[k].desc, self.slots.kinds()[k]) for k in bad[:3]])

    def where(self, at):
        k = max(int(np.searchsorted(self.slots.offsets, self.slots.lo + int(at), side="right")) - 1, 0)
        return f"slot of chain {k} ({self.chains[k].desc}) + {self.slots.lo + int(at) - int(self.slots.offsets[k])}"


@pytest.fixture(params=[(False, True, True), (True, True, True), (True, True, False), (True, False, True),
                        (True, False, False)],
                ids=["unfused-lines+flat", "fused-lines+flat", "fused-lines", "fused-flat", "fused-scan"])
def route(request):
    fused, lines, flat = request.param
    before = H.set_b64_fused(fused), H.set_b64_lines(lines), H.set_b64_flat(flat)
    yield request.param
    H.set_b64_fused(before[0])
    H.set_b64_lines(before[1])
    H.set_b64_flat(before[2])


@pytest.mark.parametrize("slot_mode", [L.AT, L.STRADDLE])
def test_text_and_slots_past_the_line(route, slot_mode, big, big2):
    """lbf_b64_update_launch with `out` and `text` of 4 GiB and a window each:
    slots below, across or exactly at, and above byte 2^32 at the phases 0, 5 and
    15, pieces on both sides of byte 2^32 of the text, one across it or exactly
    at it in every round.  After every launch: every byte of the slots' window,
    0xEE at the same positions minus 2^32, both record arrays, lengths, verdicts
    and digests (which show the piece table the hash read)."""
    feed = WindowFeed(_text_chains(), slot_mode, big, big2)
    try:
        for r in range(feed.rounds):
            feed.run_round(r)
        n = len(feed.chains)
        assert feed.d_b64.download(16 * n).tobytes() == new_b64_states(n).tobytes()
        assert feed.d_sha.download(96 * n).tobytes() == new_states(n).tobytes()
    finally:
        feed.close()


# ------------------------------------------------------------ f. more than 65,536 chains, the table form
@pytest.fixture(scope="module")
def count():
    return L.entry_count()


@pytest.fixture(scope="module")
def many(oracle, count):
    data, offs, sizes = L.small_table(count, 6500)
    return data, offs, sizes, _frozen(oracle.sha1_batch(data, offs, sizes, nthreads=8))


def test_more_entries_than_the_threshold_table_form(forced, many, count):
    """lbf_sha1_launch with the threshold + 64 + 37 chains of 0..200 bytes at
    unaligned offsets in one launch: digests, nothing written past entry
    `count`, and verdicts with flips on both sides of entry 65,536."""
    data, offs, sizes, want = many
    n, room = count, count + 128
    describe = lambda i: f"entry {int(i)} of {n}: size {int(sizes[i])}, offset {int(offs[i])}"  # noqa: E731
    flips = [0, 65535, 65536, n - 1]
    exp = np.full((room, 20), FILL, dtype=np.uint8)
    exp[:n] = _flip_expected(want.copy(), flips)
    with Device() as dev:
        d_data, d_off, d_size = dev.put(data), dev.put(offs), dev.put(sizes)
        d_dig, d_exp, d_ver = dev.filled(20 * room), dev.put(exp), dev.filled(room)
        H.batch_launch(d_data, d_off, d_size, n, d_dig)
        H.synchronize()
        dig = d_dig.download(20 * room)
        _assert_rows(dig[:20 * n].reshape(n, 20), want, describe, "digests")
        assert (dig[20 * n:] == FILL).all(), "digest bytes written past the last entry"
        H.batch_launch(d_data, d_off, d_size, n, None, expected=d_exp, verdicts=d_ver)
        H.synchronize()
        ver = d_ver.download(room)
        _assert_rows(ver[:n], _verdict_pattern(n, flips), describe, "verdicts")
        assert (ver[n:] == FILL).all(), "verdict bytes written past the last entry"


# ------------------------------------------------------------ g. more than 65,536 pieces, resumable SHA-1
def _documented_update_mb():
    """The default of LBF_UPDATE_MB as include/lbf_hash.h documents it."""
    with open(os.path.join(ROOT, "include", "lbf_hash.h")) as f:
        m = re.search(r"at most LBF_UPDATE_MB MiB of piece bytes\s*\n\s*\* \(default (\d+),", f.read())
    return int(m.group(1))


@pytest.fixture(scope="module")
def pieces(oracle, count):
    """`count` chains of two touching pieces of 0..200 bytes each.  Every even
    chain ends with its first piece, so its second piece is a chunk of its own."""
    rng = np.random.default_rng(6600)
    data, offs, sizes = L.small_table(count, 6601, top=400)
    a = np.minimum(rng.integers(0, 201, count), sizes).astype(np.uint32)
    b = np.minimum(sizes - a, 200).astype(np.uint32)
    off2 = offs + a
    final1 = (np.arange(count) % 2 == 0).astype(np.uint8)
    perm = rng.permutation(count).astype(np.uint32)
    d1 = oracle.sha1_batch(data, offs, a, nthreads=8)                       # of the first piece alone
    d2 = oracle.sha1_batch(data, off2, b, nthreads=8)                      # of the second alone
    d12 = oracle.sha1_batch(data, offs, a + b, nthreads=8)                 # of both
    want2 = np.where((perm % 2 == 0)[:, None], d2[perm], d12[perm])
    return dict(data=data, off1=offs, a=a, off2=off2[perm], b=b[perm], final1=final1, perm=perm, d1=_frozen(d1),
                want2=_frozen(want2), total=int(a.sum()) + int(b.sum()))


def _check_first_call(p, dig, states, n):
    fin = p["final1"].astype(bool)
    assert np.array_equal(dig[:n][fin], p["d1"][fin])
    assert (dig[:n][~fin] == EE).all() and (dig[n:] == EE).all(), "a digest entry of a piece that is not final written"
    assert states[fin].tobytes() == new_states(int(fin.sum())).tobytes()
    assert np.array_equal(states["total"][~fin], p["a"][~fin])
    assert np.array_equal(states["buffered"], states["total"] % 64)


def test_more_pieces_than_the_threshold_update_chunks(hasher, pieces, count):
    """update_chunks with threshold + 64 + 37 pieces in one call, twice: half
    the chains final in the first call, state_of a permutation in the second.
    One launch each: the call's bytes are far below LBF_UPDATE_MB."""
    p, n = pieces, count
    mb = int(os.environ.get("LBF_UPDATE_MB") or _documented_update_mb())
    assert _documented_update_mb() == 256 and p["total"] < (mb << 20) // 8, "more than one launch"
    states = new_states(n)
    dig = np.full((n + 16, 20), EE, dtype=np.uint8)
    buf = p["data"]
    assert _raw_update(hasher, states, buf, p["off1"], p["a"], None, p["final1"], dig, None, None) == 0
    _check_first_call(p, dig, states, n)
    dig[:] = EE
    assert _raw_update(hasher, states, buf, p["off2"], p["b"], p["perm"], np.ones(n, np.uint8), dig, None, None) == 0
    bad = np.flatnonzero((dig[:n] != p["want2"]).any(axis=1))
    assert bad.size == 0, (bad.size, bad[:8].tolist())
    assert (dig[n:] == EE).all()
    assert states.tobytes() == new_states(n).tobytes()


def test_more_pieces_than_the_threshold_update_launch(pieces, count):
    """The same two rounds through lbf_sha1_update_launch, everything in device
    buffers: the 256-thread geometry of the update kernel."""
    p, n = pieces, count
    with Device() as dev:
        d_states, d_data = dev.put(new_states(n + 1)), dev.put(p["data"])
        d_dig = dev.put(np.full(20 * (n + 16), EE, dtype=np.uint8))
        d_off, d_size, d_fin = dev.put(p["off1"]), dev.put(p["a"]), dev.put(p["final1"])
        H.update_launch(d_states, n, None, d_data, d_off, d_size, d_fin, n, d_dig)
        H.synchronize()
        states = d_states.download(96 * (n + 1)).view(STATE_DTYPE)
        _check_first_call(p, d_dig.download(20 * (n + 16)).reshape(-1, 20), states[:n], n)
        d_dig.upload(np.full(20 * (n + 16), EE, dtype=np.uint8))
        d_off2, d_size2 = dev.put(p["off2"]), dev.put(p["b"])
        d_so, d_fin2 = dev.put(p["perm"]), dev.put(np.ones(n, dtype=np.uint8))
        H.update_launch(d_states, n, d_so, d_data, d_off2, d_size2, d_fin2, n, d_dig)
        H.synchronize()
        dig = d_dig.download(20 * (n + 16)).reshape(-1, 20)
        bad = np.flatnonzero((dig[:n] != p["want2"]).any(axis=1))
        assert bad.size == 0, (bad.size, bad[:8].tolist())
        assert (dig[n:] == EE).all()
        assert d_states.download(96 * (n + 1)).tobytes() == new_states(n + 1).tobytes()


# ------------------------------------------------------------ h. more than 65,536 pieces of text
@functools.lru_cache(maxsize=None)
def _slices(n):
    c = W.slices_corpus()
    assert len(c) >= n
    texts, chunks = c.texts[:n], c.chunks[:n]
    expected = c.expected()[:n]
    exp = digests_of(chunks).copy()
    exp[~np.array(c.digest_ok[:n], dtype=bool), 0] ^= 1
    return texts, chunks, expected, exp


@pytest.mark.parametrize("fused", [False, True], ids=["unfused-default", "fused-lines+flat"])
def test_more_pieces_than_the_threshold_update_text(hasher, count, fused):
    """update_text with threshold + 64 + 37 texts of 0..60-byte chunks as one
    final piece each, one launch; then each text cut in two inside its first
    group.  Verdicts, lengths and every byte of the arena against the models:
    b64_length_kernel and the per-piece grids past entry 65,535."""
    n = count
    texts, chunks, expected, exp = _slices(n)
    before = [H.set_b64_fused(fused)] + ([H.set_b64_lines(True), H.set_b64_flat(True)] if fused else [])
    try:
        tlen = np.array([len(t) for t in texts], dtype=np.uint32)
        toff = (np.cumsum(tlen + 3, dtype=np.uint64) - tlen).astype(np.uint64)
        text = np.full(int(toff[-1]) + int(tlen[-1]) + 16, ord("A"), dtype=np.uint8)
        for o, t in zip(toff.tolist(), texts):
            text[o:o + len(t)] = np.frombuffer(t, dtype=np.uint8)
        caps = np.array([len(d) for d in chunks], dtype=np.uint32)
        ooff = (np.cumsum(caps + np.arange(n, dtype=np.uint32) % 3, dtype=np.uint64) - caps + 5).astype(np.uint64)
        want_out = np.full(int(ooff[-1]) + int(caps[-1]) + 16, EE, dtype=np.uint8)
        for o, (w, _, _) in zip(ooff.tolist(), expected):
            want_out[o:o + len(w)] = np.frombuffer(w, dtype=np.uint8)
        want_size = np.array([s for _, s, _ in expected], dtype=np.uint32)
        want_ver = np.array([v for _, _, v in expected], dtype=bool)
        assert want_ver.sum() > n // 2 and (~want_ver).sum() > n // 12
        cut = np.minimum(1 + np.arange(n) % 2, tlen).astype(np.uint32)   # inside the first group, in front of any '='
        for cuts in (None, cut):
            b64, sha = new_b64_states(n), new_states(n)
            out = np.full(want_out.size, EE, dtype=np.uint8)
            if cuts is not None:
                sizes, ver = hasher.update_text(b64, sha, text, toff, cuts, out, ooff, caps, expected=exp)
                assert not sizes.any() and not ver.any() and (out == EE).all()
                assert not b64["decoded"].any() and not b64["ended"].any() and not sha["total"].any()
                alpha = np.array([sum(ch in W.ALPHABET for ch in t[:int(a)]) for t, a in zip(texts, cuts)])
                eq = np.array([b"=" in t[:int(a)] for t, a in zip(texts, cuts)])
                assert not eq.any() and np.array_equal(b64["ncarry"], alpha)
            a = np.zeros(n, dtype=np.uint32) if cuts is None else cuts
            state_of = None if cuts is None else np.arange(n, dtype=np.uint32)
            sizes, ver = hasher.update_text(b64, sha, text, toff + a, tlen - a, out, ooff, caps, state_of=state_of,
                                            final=np.ones(n), expected=exp)
            what = "whole" if cuts is None else "cut in two"
            bad = np.flatnonzero(sizes != want_size)
            assert bad.size == 0, (what, "lengths", bad[:8].tolist())
            bad = np.flatnonzero(ver != want_ver)
            assert bad.size == 0, (what, "verdicts", bad[:8].tolist())
            bad = np.flatnonzero(out != want_out)
            assert bad.size == 0, (what, "arena", bad[:8].tolist(), int(np.searchsorted(ooff, bad[:1], "right")[0]) - 1)
            assert b64.tobytes() == new_b64_states(n).tobytes() and sha.tobytes() == new_states(n).tobytes()
    finally:
        H.set_b64_fused(before[0])
        if fused:
            H.set_b64_lines(before[1])
            H.set_b64_flat(before[2])


# ------------------------------------------------------------ i. host arrays of more than 4 GiB
HOST_BYTES = LINE + (1 << 20)


def test_update_chunks_over_a_host_array_past_4gib(hasher):
    """update_chunks with pieces on both sides of byte 2^32 of a host array of
    2^32 + 1 MiB bytes, touched only around the line and in its last MiB."""
    rng = np.random.default_rng(4096)
    buf = np.zeros(HOST_BYTES, dtype=np.uint8)
    buf[LINE - 4096:LINE + 4096] = rng.integers(0, 256, 8192, dtype=np.uint8)
    buf[:4096] = rng.integers(0, 256, 4096, dtype=np.uint8)       # what offsets taken mod 2^32 would read
    buf[-(1 << 20):] = rng.integers(0, 256, 1 << 20, dtype=np.uint8)
    off1 = [LINE - 70, LINE - 6, LINE + 64, LINE, HOST_BYTES - 5000, 7, LINE - 3000]
    sz1 = [64, 70, 100, 33, 4000, 100, 2999]
    off2 = [LINE - 6, LINE + 64, HOST_BYTES - 129, LINE + 1, LINE - 1, LINE + 15, LINE + 8]
    sz2 = [70, 1000, 129, 0, 2, 3000, 56]
    n = len(off1)
    assert {L.kind_of(o, s) for o, s in zip(off1 + off2, sz1 + sz2)} == {L.BELOW, L.STRADDLE, L.AT, L.ABOVE}
    states = new_states(n)
    out = hasher.update_chunks(states, buf, off1, sz1)
    assert not out.any()
    p1 = [buf[o:o + s].tobytes() for o, s in zip(off1, sz1)]
    assert not M.sha_records_differ(states, _mid_records(p1))
    perm = rng.permutation(n)
    got = hasher.update_chunks(states, buf, np.array(off2)[perm], np.array(sz2)[perm], state_of=perm, final=np.ones(n))
    want = digests_of(p1[k] + buf[off2[k]:off2[k] + sz2[k]].tobytes() for k in perm)
    assert np.array_equal(got, want), np.flatnonzero((got != want).any(axis=1)).tolist()
    assert states.tobytes() == new_states(n).tobytes()
    # the bounds check at 64-bit lengths: a piece that ends one byte past the array
    with pytest.raises(H.LbfError):
        hasher.update_chunks(states, buf, [HOST_BYTES - 10], [11], state_of=[0])


@pytest.mark.parametrize("fused", [False, True], ids=["unfused", "fused"])
def test_update_text_over_host_arrays_past_4gib(hasher, fused):
    """update_text with the text and the slots on both sides of byte 2^32 of
    host arrays of 2^32 + 1 MiB bytes; only the windows are looked at."""
    chains = [c for c in _text_chains()][:10]
    n = len(chains)
    caps = [c.cap for c in chains]
    slots = L.slot_case(caps, _anchor(caps), L.STRADDLE, EE)
    assert slots.alloc <= HOST_BYTES
    out = np.zeros(HOST_BYTES, dtype=np.uint8)
    text = np.zeros(HOST_BYTES, dtype=np.uint8)
    out[slots.lo:slots.hi] = EE
    out[:slots.alias.size] = EE
    want = slots.window.copy()
    b64, sha = new_b64_states(n), new_states(n)
    model, sofar = [M.init()] * n, [b""] * n
    exp = np.frombuffer(b"".join(c.expected for c in chains), dtype=np.uint8).reshape(n, 20)
    before = H.set_b64_fused(fused)
    try:
        for r in range(3):
            lens = [len(c.pieces[r]) for c in chains]
            t = L.text_case(lens, _anchor(lens), (L.AT, L.STRADDLE)[r % 2], phase=5, seed=200 + r)
            assert t.alloc <= HOST_BYTES
            for j, c in enumerate(chains):
                a = int(t.offsets[j]) - t.lo
                t.window[a:a + lens[j]] = np.frombuffer(c.pieces[r], dtype=np.uint8)
            text[:t.alias.size] = t.alias
            text[t.lo:t.hi] = t.window
            fin = np.full(n, r == 2)
            sizes, ver = hasher.update_text(b64, sha, text, t.offsets, lens, out, slots.offsets, slots.sizes, final=fin,
                                            expected=exp)
            for k, c in enumerate(chains):
                was = len(sofar[k])
                if r == 2:
                    model[k], sofar[k] = M.init(), c.want
                    assert sizes[k] == c.size and bool(ver[k]) == c.verdict, (c.desc, int(sizes[k]), c.size)
                else:
                    model[k], new = model_update(model[k], c.pieces[r])
                    sofar[k] += new
                    assert sizes[k] == 0 and not ver[k]
                s, a, b = int(slots.offsets[k]) - slots.lo, min(was, c.cap), min(len(sofar[k]), c.cap)
                want[s + a:s + b] = np.frombuffer(sofar[k][a:b], dtype=np.uint8)
            wrong = np.flatnonzero(out[slots.lo:slots.hi] != want)
            assert wrong.size == 0, (r, "byte 2^32%+d" % (slots.lo + int(wrong[0]) - LINE))
            assert (out[:slots.alias.size] == EE).all(), (r, "a slot position taken mod 2^32")
            assert not out[slots.alias.size:slots.alias.size + 4096].any() and not out[slots.hi:slots.hi + 4096].any()
            assert b64.tobytes() == M.b64_records(model, B64_STATE_DTYPE).tobytes(), r
    finally:
        H.set_b64_fused(before)
    assert sha.tobytes() == new_states(n).tobytes()

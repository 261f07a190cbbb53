"""The layouts of tests/large_index.py reach what they are built to reach.

No GPU.  tests/test_gpu_large_index.py relies on these conditions when it calls
a green run proof that no address expression of a launch path is kept in 32
bits: every entry that touches byte 2^32 or lies past it has, at its positions
mod 2^32, other bytes (reads) or the fill value (writes) inside the same
allocation, so a truncated address gives a wrong answer and never a fault; each
case holds entries below, across, exactly at and above the line, the ones above
at the start residues 1, 5, 15 and 8 mod 16; and the entry counts lie past the
threshold the launchers switch their workgroup size at, which is read from the
sources here.
"""
import hashlib

import numpy as np
import pytest

from tests import large_index as L
from tests import wire_flat_model as F
from tests.test_gpu_update import FIRST, SECOND

LINE = L.LINE


def _check_ranges(r, disjoint=False):
    assert r.offsets.dtype == np.uint64 and r.sizes.dtype == np.uint32 and r.offsets.size == r.sizes.size
    assert r.lo % 16 == 0 and 0 < r.lo < LINE < r.hi == r.alloc
    ends = r.offsets.astype(np.int64) + r.sizes
    assert int(r.offsets.min()) >= r.lo and int(ends.max()) <= r.hi
    # the alias window covers every position past the line, minus 2^32, and ends below the high window
    assert r.alias.size == r.hi - LINE and r.alias.size < r.lo
    assert r.window.size + r.alias.size < 8 << 20, "the windows stay small"
    for o, e in zip(r.offsets.tolist(), ends.tolist()):
        if e >= LINE:  # touches the line or lies past it: its positions mod 2^32 are inside the allocation
            a, b = (o % LINE, e % LINE) if o >= LINE else (0, e - LINE)
            assert 0 <= a <= b <= r.alias.size <= r.alloc
    if disjoint:
        order = np.argsort(r.offsets, kind="stable")
        assert (r.offsets[order][1:].astype(np.int64) >= ends[order][:-1]).all(), "ranges overlap"
    up = list(r.uploads())
    assert [(o, b.size) for o, b in up] == [(0, r.alias.size), (r.lo, r.window.size)]


def _check_kinds(r, phases=L.ABOVE_PHASES):
    kinds = r.kinds()
    assert {L.BELOW, L.STRADDLE, L.AT, L.ABOVE} <= set(kinds), set(kinds)
    for o, s, k in zip(r.offsets.tolist(), r.sizes.tolist(), kinds):
        assert k == {True: L.AT, False: L.ABOVE if o > LINE else L.STRADDLE if o + s > LINE else L.BELOW}[o == LINE]
    above = {int(o) % 16 for o, k in zip(r.offsets, kinds) if k == L.ABOVE}
    assert set(phases) <= above, above
    return kinds


def _check_reads_differ(r):
    """A truncating reader sees other bytes: entry by entry, wherever the true
    range holds a byte at or past the line."""
    for i, (o, s) in enumerate(zip(r.offsets.tolist(), r.sizes.tolist())):
        if s and o + s > LINE:
            assert r.truncated_bytes(i) != r.true_bytes(i), (i, o, s)
            assert hashlib.sha1(r.truncated_bytes(i)).digest() != hashlib.sha1(r.true_bytes(i)).digest()
        else:
            assert r.truncated_bytes(i) == r.true_bytes(i)


def test_place():
    sizes = [100, 0, 33, 200, 7, 1000, 64]
    phases = [3, 9, 15, 0, 1, 8, 5]
    for anchor, mode in ((3, L.AT), (3, L.STRADDLE), (5, L.STRADDLE), (0, L.AT), (5, L.STRADDLE)):
        ph = list(phases)
        if mode == L.AT:
            ph[anchor] = 0
        st = L.place(sizes, ph, anchor, mode).astype(np.int64)
        assert [int(x) % 16 for x in st] == ph
        assert all(st[k] + sizes[k] <= st[k + 1] < st[k] + sizes[k] + 32 for k in range(len(sizes) - 1))
        assert L.kind_of(int(st[anchor]), sizes[anchor]) == mode
        assert all(L.kind_of(int(st[k]), sizes[k]) == L.BELOW for k in range(anchor))
        assert all(L.kind_of(int(st[k]), sizes[k]) == L.ABOVE for k in range(anchor + 1, len(sizes)))
    with pytest.raises(ValueError):
        L.place(sizes, phases, 2, L.STRADDLE)
    with pytest.raises(ValueError):
        L.place(sizes, phases, 0, L.AT)


def test_table_case():
    r = L.table_case()
    assert 195 <= r.n <= 210 and int(r.sizes.max()) == 3000 and int(r.sizes.min()) == 0
    _check_ranges(r)
    kinds = _check_kinds(r)
    _check_reads_differ(r)
    assert sum(k == L.STRADDLE for k in kinds) >= 5 and sum(k == L.BELOW for k in kinds) >= 50
    # both tail forms of the padding on both sides of the line
    for side in (L.BELOW, L.ABOVE):
        tails = {int(s) & 63 >= 56 for s, k in zip(r.sizes, kinds) if k == side}
        assert tails == {False, True}, side
    # shuffled: every wave of 64 entries mixes entries below and above the line
    for w0 in range(0, r.n, 64):
        assert {L.BELOW, L.ABOVE} <= set(kinds[w0:w0 + 64]), w0


def test_uniform_cases():
    cases = L.uniform_cases()
    assert [cs % 2 for cs, *_ in cases] == [1, 0] and cases[1][0] % 16 == 0
    for cs, first, n, length in cases:
        assert first * cs < LINE < (first + n) * cs
        assert 130 <= n <= 200 and n > 128 and n % 64
        assert 0 < length - (first + n - 1) * cs < cs, "the last chunk is short"
        r = L.uniform_ranges(cs, first, n, length)
        _check_ranges(r, disjoint=True)
        assert r.hi >= length and int(r.offsets[0]) == first * cs and r.n == n
        assert int(r.sizes[-1]) == length - (first + n - 1) * cs and (r.sizes[:-1] == cs).all()
        _check_reads_differ(r)
        kinds = r.kinds()
        assert {L.BELOW, L.ABOVE} <= set(kinds) and (L.STRADDLE in kinds) != (L.AT in kinds)
        # and from one chunk later, the sub-range the GPU test also launches
        assert (first + 1) * cs < LINE
    odd, even = cases
    starts = {((odd[1] + i) * odd[0]) % 16 for i in range(odd[2]) if (odd[1] + i) * odd[0] > LINE}
    assert starts == set(range(16)), "an odd chunk size meets every residue above the line"
    assert L.STRADDLE in L.uniform_ranges(*odd).kinds()
    assert L.AT in L.uniform_ranges(*even).kinds() and LINE % even[0] == 0


def test_piece_cases():
    combos = L.thinned(FIRST, SECOND)
    assert 55 <= len(combos) <= 65
    assert {a for a, _ in combos} == set(FIRST) and {b for _, b in combos} == set(SECOND)
    first, second = L.piece_cases([a for a, _ in combos], [b for _, b in combos])
    assert first.window is second.window and first.lo == second.lo
    for r in (first, second):
        _check_ranges(r, disjoint=True)
        _check_reads_differ(r)
        assert {int(o) % 16 for o in r.offsets} == {0, 1, 8, 15}
        kinds = r.kinds()
        assert {L.BELOW, L.ABOVE} <= set(kinds)
        above = {int(o) % 16 for o, k, s in zip(r.offsets, kinds, r.sizes) if k == L.ABOVE and s}
        assert above == {0, 1, 8, 15}
    assert L.AT in first.kinds() and L.STRADDLE in second.kinds()


def test_state_indices():
    B = L.STATE_BYTES
    assert L.S == 44_739_243 and (L.S - 1) * B < LINE <= L.S * B
    kinds = [L.kind_of(i * B, B) for i in L.STATE_INDICES]
    assert kinds == [L.BELOW, L.STRADDLE, L.ABOVE, L.ABOVE, L.ABOVE]
    assert L.S * B - LINE < B  # the first record past the line starts less than a record behind it
    assert L.N_STATES > max(L.STATE_INDICES + (L.STATE_NEIGHBOUR,)) and L.N_STATES * B < LINE + (1 << 16)
    # the alias bytes: the same byte positions minus 2^32, far below the records in use
    for i in L.STATE_INDICES + (L.STATE_NEIGHBOUR,):
        a = i * B + B - LINE
        assert a <= 0 or a <= L.N_STATES * B - LINE < (L.S - 2) * B
    assert L.STATE_NEIGHBOUR not in L.STATE_INDICES


@pytest.mark.parametrize("mode", [L.AT, L.STRADDLE])
def test_slot_and_text_cases(mode):
    big = 5 * F.TILE_BYTES + 1000
    caps = [big] * 8 + [0, 1, 2, 3, 55, 57, 58, 864] + [big] * 8
    anchor = 3
    r = L.slot_case(caps, anchor, mode, 0xEE)
    _check_ranges(r, disjoint=True)
    kinds = r.kinds()
    assert kinds[anchor] == mode and {L.BELOW, L.ABOVE} <= set(kinds)
    above = {int(o) % 16 for o, k in zip(r.offsets, kinds) if k == L.ABOVE}
    assert {0, 5, 15} <= above
    assert (r.window == 0xEE).all() and (r.alias == 0xEE).all()
    lens = [100, 5000, 7, 30000, 0, 5256, 64]
    t = L.text_case(lens, 3, mode, phase=9, seed=5)
    _check_ranges(t, disjoint=True)
    _check_reads_differ(t)
    assert t.kinds()[3] == mode and {L.BELOW, L.ABOVE} <= set(t.kinds())
    alphabet = set(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/")
    assert set(t.window.tolist()) <= alphabet and set(t.alias.tolist()) <= alphabet


def test_entry_count_from_the_sources():
    g = L.launch_geometry()
    assert g["lane"] == (65536, 64, 256) and g["update"] == (65536, 64, 256)
    assert g["length"] == (256, 255, 256, 256)
    n = L.entry_count()
    assert n == 65536 + 64 + 37
    lo, hi = g["lane"][1], g["lane"][2]
    assert n > g["lane"][0] and (n - g["lane"][0]) // lo == 1 and (n - g["lane"][0]) % lo == 37
    # in blocks of 256: the last workgroup has one full wave, one partial wave and two idle ones
    last = n % hi
    assert last // 64 == 1 and 0 < last % 64 < 64 and hi // 64 - (last + 63) // 64 == 2
    assert n > 65535, "past a 16-bit entry index and past grid.y's limit"


def test_small_table():
    n = 1000
    data, offs, sizes = L.small_table(n, 3)
    ends = offs.astype(np.int64) + sizes
    assert int(sizes.min()) == 0 and int(sizes.max()) == 200 and int(ends.max()) <= data.size
    assert (offs[1:].astype(np.int64) >= ends[:-1]).all()
    assert len({int(o) % 16 for o in offs}) == 16

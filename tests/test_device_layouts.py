"""The layouts of tests/device_layouts.py reach what they are built to reach.

No GPU.  The loop model (device_layouts.loop_model) restates the fast-loop
bound of the producer/consumer kernels; the conditions below are what
tests/test_gpu_device_paths.py relies on when it calls 26 block steps enough:
every exit residue of both unrolls after at least two full trips, every way a
short chain can end inside or just behind the fast loop, every start residue
mod 16 and every tail edge.  The oracle the GPU tests compare with is pinned
here against hashlib on one of the tables.
"""
import hashlib

import numpy as np
import pytest

from tests import device_layouts as L

# (steps per fast-loop trip, chains per workgroup): pc4; pc4x2 and pcx5
GEOMETRIES = [(8, 64), (6, 128)]
GEO_IDS = ["pc4-U8-64", "pc4x2.pcx5-U6-128"]


@pytest.fixture(scope="module")
def level64():
    return L.level_table(64)


@pytest.fixture(scope="module")
def level128():
    return L.level_table(128)


@pytest.fixture(scope="module")
def ragged():
    return L.ragged_table()


def _runs_of(table, first, count):
    return [r for r in table.runs if r.start < first + count and first < r.start + r.count]


def _check_table(t):
    n = t.n
    assert t.sizes.size == n and t.offsets.dtype == np.uint64 and t.sizes.dtype == np.uint32
    assert sum(r.count for r in t.runs) == n
    assert [r.start for r in t.runs] == list(np.cumsum([0] + [r.count for r in t.runs[:-1]]))
    ends = t.offsets.astype(np.int64) + t.sizes
    assert int(ends.max()) <= t.data.size
    order = np.argsort(t.offsets, kind="stable")
    assert (t.offsets[order][1:].astype(np.int64) >= ends[order][:-1]).all(), "chains overlap"
    assert t.data.size <= 16 << 20
    assert int(t.totals().max()) <= L.TMAX + 1


def test_step_formula():
    for s in [0, 1, 55, 56, 63, 64, 119, 120, 127, 128]:
        padded = s + 1 + 8  # the 0x80 byte and the 64-bit length
        assert L.steps(s) == (padded + 63) // 64, s
    for T in range(1, 30):
        for r in range(64):
            if r >= 56 and T < 2:
                with pytest.raises(ValueError):
                    L.size_for(T, r)
                continue
            s = L.size_for(T, r)
            assert L.steps(s) == T and s & 63 == r


def test_loop_model():
    # 64 per workgroup: each 64 on its own
    t = [5] * 64 + [9] * 63 + [2] + [7]
    got = [(c.first, c.live, c.nsteps, c.min_steps, c.fast_end) for c in L.loop_model(t, 64)]
    assert got == [(0, 64, 5, 5, 4), (64, 64, 9, 2, 2), (128, 1, 7, 7, 6)]
    # 128 per workgroup: nsteps over both groups, min_steps per group
    got = [(c.first, c.live, c.nsteps, c.min_steps, c.fast_end) for c in L.loop_model(t, 128)]
    assert got == [(0, 64, 9, 5, 5), (64, 64, 9, 2, 2), (128, 1, 7, 7, 6)]
    assert L.loop_model([20] * 64, 64)[0].fast_trips(8) == 2
    assert L.loop_model([1] * 3, 128)[0].fast_end == 0


@pytest.mark.parametrize("group", [64, 128])
def test_level_table_structure(group, level64, level128):
    tables = level64 if group == 64 else level128
    assert len(tables) == (2 if group == 64 else 1)
    for t in tables:
        _check_table(t)
        seen = set()
        for run in t.runs:
            sl = slice(run.start, run.start + run.count)
            assert run.count == group
            assert (t.sizes[sl] == L.size_for(run.T, run.r)).all()
            res = t.offsets[sl].astype(np.int64) % 16
            if run.align == L.WALK:
                assert (res == np.arange(group) % 16).all()
            else:
                assert (res == run.align).all()
            seen.add((run.T, run.r, run.align))
        for align in L.ALIGNS:
            for T in range(1, L.TMAX + 1):
                assert (T, L.TAIL_ONE, align) in seen
                assert T == 1 or (T, L.TAIL_TWO, align) in seen
                for r in L.TAILS_LOW_T:
                    assert ((T, r, align) in seen) == (T <= 9)
    if group == 64:
        a, b = tables
        key = lambda r: (r.T, r.r, r.align)  # noqa: E731
        assert [key(r) for r in b.runs] == [key(r) for r in a.runs[1:] + a.runs[:1]]


def _level_consumers(tables, per_wg):
    """(consumer, tail residue, alignment) of every consumer whose whole
    workgroup lies in runs of one tail form and one alignment."""
    out = []
    for t in tables:
        for c in L.loop_model(t.totals(), per_wg):
            runs = _runs_of(t, c.first - c.first % per_wg, per_wg)
            kinds = {(r.r, r.align) for r in runs}
            if len(kinds) == 1:
                out.append((c,) + kinds.pop())
    return out


@pytest.mark.parametrize("U,per_wg", GEOMETRIES, ids=GEO_IDS)
def test_level_tables_reach_every_exit_residue_after_two_trips(U, per_wg, level64, level128):
    sets = [("level128", level128)]
    if per_wg == 64:
        sets += [("level64/0", level64[:1]), ("level64/1", level64[1:])]
    else:
        sets += [("level64, both orderings", level64)]
    for name, tables in sets:
        cons = _level_consumers(tables, per_wg)
        for r in (L.TAIL_ONE, L.TAIL_TWO):
            for align in L.ALIGNS:
                got = {c.nsteps % U for c, cr, ca in cons if cr == r and ca == align and c.fast_end >= 2 * U}
                assert got == set(range(U)), (name, L.tail_form(r), align, sorted(got))
    # three trips of U = 8 and four of U = 6 happen too
    most = max(c.fast_trips(U) for c, _, _ in _level_consumers(level128, per_wg))
    assert most == (3 if U == 8 else 4)


def test_level64_orderings_pair_consecutive_step_counts(level64):
    """128-chain workgroups of the two orderings hold (T, T+1) for every T in
    1..25, in both tail forms (two-block from T = 2) and both alignments."""
    pairs = set()
    for t in level64:
        for w0 in range(0, t.n, 128):
            runs = _runs_of(t, w0, 128)
            if len(runs) == 2 and (runs[0].r, runs[0].align) == (runs[1].r, runs[1].align):
                pairs.add((runs[0].T, runs[1].T, runs[0].r, runs[0].align))
    for align in L.ALIGNS:
        for T in range(1, L.TMAX):
            assert (T, T + 1, L.TAIL_ONE, align) in pairs
            assert T == 1 or (T, T + 1, L.TAIL_TWO, align) in pairs


def test_ragged_table_structure(ragged):
    _check_table(ragged)
    want = []
    for ts in range(1, 21):
        for tl in sorted({ts + 1, ts + 2, ts + 7, L.TMAX}):
            want += [(ts, tl, False), (ts, tl, True)]
    got = []
    for run in ragged.runs:
        sl = slice(run.start, run.start + run.count)
        assert run.count == 64
        t = ragged.totals()[sl]
        long = np.arange(64) != L.SHORT_LANE
        assert (t[long] == run.T).all() and t[L.SHORT_LANE] == run.T_short < run.T
        assert (ragged.sizes[sl][long] & 63 == run.r).all()
        assert ragged.sizes[sl][L.SHORT_LANE] & 63 == run.r_short
        res = ragged.offsets[sl].astype(np.int64) % 16
        assert (res[long] == 0).all() and res[L.SHORT_LANE] == run.short_align
        got.append((run.T_short, run.T, run.short_align != 0))
    assert got == want


@pytest.mark.parametrize("U,per_wg", GEOMETRIES, ids=GEO_IDS)
def test_ragged_table_reaches_every_short_chain_exit(U, per_wg, ragged):
    """Every (min_steps mod U, how far nsteps lies past min_steps: 1, 2, 3 or
    more) after at least one full trip of the fast loop, with the short chain
    aligned and misaligned."""
    totals = ragged.totals()
    for mis in (False, True):
        got = set()
        for c in L.loop_model(totals, per_wg):
            run = ragged.run_of(c.first)
            if (run.short_align != 0) == mis and c.fast_end >= U:
                assert c.min_steps == run.T_short
                got.add((c.min_steps % U, min(c.nsteps - c.min_steps, 3)))
        assert got == {(m, d) for m in range(U) for d in (1, 2, 3)}, (mis, sorted(got))


def test_every_table_has_every_start_residue_and_tail_edge(level64, level128, ragged):
    for t in level64 + level128 + [ragged]:
        assert set((t.offsets.astype(np.int64) % 16).tolist()) == set(range(16)), t.name
        assert set(L.EDGE_TAILS) <= set((t.sizes & 63).tolist()), t.name


def test_uniform_cases():
    cases = L.uniform_cases()
    assert len(cases) == len(set(cases)) == 2 * 3 * (2 * L.TMAX - 1) + 3
    assert sum(1 for c in cases if c[1] == 65) == 3
    residues, tails, combos, by_t = set(), set(), set(), set()
    reach = {}
    for cs, n, length, shift in cases:
        assert n in (64, 65, 128, 129) and shift in (0, 3)
        short = length - (n - 1) * cs
        assert short in (1, cs - 1, cs) and (length + cs - 1) // cs == n
        offs, sizes = L.uniform_table(cs, n, length)
        assert int(offs[-1]) + int(sizes[-1]) == length and (sizes[:-1] == cs).all() and sizes[-1] == short
        assert L.steps(cs) <= L.TMAX
        residues |= set(((offs.astype(np.int64) + shift) % 16).tolist())
        tails |= set((sizes & 63).tolist())
        rounded = cs % 16 == 0
        if n != 65:
            assert rounded or cs % 2 == 1
            combos.add((rounded, n, (1, cs - 1, cs).index(short), shift))
            by_t.add((rounded, L.steps(cs), L.tail_form(cs & 63)))
        if cs % 2 == 1:  # successive chunks start at every residue mod 16
            assert set(((offs[:16].astype(np.int64) + shift) % 16).tolist()) == set(range(16))
        # what the chains of this case look like to a kernel: odd sizes by tail
        # form (mixed alignment), multiples of 16 by alignment (all or none)
        kind = ("rounded", shift) if rounded else ("odd", L.tail_form(cs & 63))
        for U, per_wg in GEOMETRIES:
            for c in L.loop_model(L.steps(sizes), per_wg):
                if c.fast_end >= 2 * U:
                    reach.setdefault((U, kind), set()).add(c.nsteps % U)
    assert residues == set(range(16))
    assert set(L.EDGE_TAILS) <= tails
    assert combos == {(ro, n, s, sh) for ro in (False, True) for n in (64, 128, 129) for s in range(3) for sh in (0, 3)}
    for T in range(1, L.TMAX + 1):
        assert (False, T, "one-block") in by_t and (T == 1 or (False, T, "two-block") in by_t)
        assert (True, T, "one-block") in by_t  # a multiple of 16 has no two-block tail
    for U, _ in GEOMETRIES:
        for kind in [("odd", "one-block"), ("odd", "two-block"), ("rounded", 0), ("rounded", 3)]:
            assert reach.get((U, kind)) == set(range(U)), (U, kind, reach.get((U, kind)))


def test_oracle_matches_hashlib_on_a_level_table(oracle, level64):
    t = level64[0]
    got = oracle.sha1_batch(t.data, t.offsets, t.sizes)
    raw = t.data.tobytes()
    for i, (o, s) in enumerate(zip(t.offsets.tolist(), t.sizes.tolist())):
        assert bytes(got[i]) == hashlib.sha1(raw[o:o + s]).digest(), t.describe(i)

"""Chunk layouts that sweep block counts and start alignment -- TEST INFRASTRUCTURE.

Pure numpy, no GPU.  tests/test_gpu_device_paths.py launches these layouts on
the device-resident entry points (lbf_sha1_uniform_launch, lbf_sha1_launch);
tests/test_device_layouts.py asserts, through the loop model at the end of
this file, that they reach what they are built to reach.

A chunk of `s` bytes takes T(s) block steps (chain_info, kern_common.hpp):

    T(s) = (s >> 6) + (2 if (s & 63) >= 56 else 1)

so a wanted T has two forms: a one-block tail, s = 64 * (T - 1) + r with r in
0..55, and (T >= 2) a two-block tail, s = 64 * (T - 2) + r with r in 56..63.

The producer/consumer kernels run an unrolled fast loop while
k + U <= fast_end, fast_end = min(min_steps, nsteps - 1) (kern_pc.hpp; pcx5
writes the same bound as two tests, kern_pcx.hpp), U = 8 for pc4 and 6 for
pc4x2 and pcx5, then a two-step tail loop.  Where the fast loop leaves off
depends on nsteps mod U and on how far min_steps lies below nsteps; the
layouts make every such exit happen after at least one full trip.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

TMAX = 26
TAIL_ONE, TAIL_TWO = 37, 61          # the two tail forms swept over every T
TAILS_LOW_T = (0, 55)                # one-block edges, for T <= 9
ALIGNS = (0, 5)                      # run start residues mod 16
EDGE_TAILS = (0, 37, 55, 56, 61, 63)
WALK = "walk"                        # a run whose chain j starts at residue j % 16
SHORT_LANE = 37


def steps(size):
    """T(s), for an int or an array."""
    s = np.asarray(size, dtype=np.int64)
    t = (s >> 6) + np.where((s & 63) >= 56, 2, 1)
    return int(t) if t.ndim == 0 else t


def size_for(T: int, r: int) -> int:
    """The chunk size with T block steps whose last partial block holds r bytes."""
    if not 0 <= r <= 63:
        raise ValueError("r must be in 0..63")
    if r >= 56:
        if T < 2:
            raise ValueError("a two-block tail needs T >= 2")
        s = 64 * (T - 2) + r
    else:
        if T < 1:
            raise ValueError("T >= 1")
        s = 64 * (T - 1) + r
    assert steps(s) == T
    return s


def tail_form(r: int) -> str:
    return "two-block" if r >= 56 else "one-block"


@dataclass
class Run:
    """`count` consecutive table entries built alike."""
    start: int
    count: int
    T: int                    # steps of the run's chains (the long ones in a ragged run)
    r: int                    # size & 63 of those chains
    align: object             # 0, 5, ... (residue mod 16 of every chain) or WALK
    T_short: int | None = None    # ragged runs: the one short chain at SHORT_LANE
    r_short: int | None = None
    short_align: int | None = None

    def describe(self, j: int) -> str:
        base = f"T={self.T} {tail_form(self.r)} tail (r={self.r}) align={self.align}"
        if self.T_short is not None:
            base += (f"; short chain at lane {SHORT_LANE}: T={self.T_short} {tail_form(self.r_short)} tail "
                     f"(r={self.r_short}) align={self.short_align}")
        return f"{base}; index {j} of {self.count} in the run"


@dataclass
class Table:
    name: str
    data: np.ndarray          # uint8, the whole buffer
    offsets: np.ndarray       # uint64
    sizes: np.ndarray         # uint32
    runs: list = field(default_factory=list)

    @property
    def n(self) -> int:
        return int(self.offsets.size)

    def totals(self) -> np.ndarray:
        return steps(self.sizes)

    def run_of(self, i: int) -> Run:
        for run in self.runs:
            if run.start <= i < run.start + run.count:
                return run
        raise IndexError(i)

    def describe(self, i: int) -> str:
        run = self.run_of(int(i))
        return f"{self.name}[{int(i)}] size {int(self.sizes[i])} offset {int(self.offsets[i])}: " \
               f"{run.describe(int(i) - run.start)}"


def _pack(name: str, specs, seed: int) -> Table:
    """specs: per run a (Run without start, [(size, residue mod 16), ...]).  Chains
    are laid one after the other in a buffer of seeded bytes, each at the next
    16-byte boundary plus its residue, so no two share a byte."""
    offs, sizes, runs = [], [], []
    pos = 0
    for run, chains in specs:
        run.start = len(offs)
        run.count = len(chains)
        for size, res in chains:
            start = (pos + 15) // 16 * 16 + res
            offs.append(start)
            sizes.append(size)
            pos = start + size
        runs.append(run)
    data = np.random.default_rng(seed).integers(0, 256, max(pos, 1), dtype=np.uint8)
    return Table(name, data, np.array(offs, dtype=np.uint64), np.array(sizes, dtype=np.uint32), runs)


def _level_run(group: int, T: int, r: int, align):
    size = size_for(T, r)
    chains = [(size, j % 16 if align == WALK else align) for j in range(group)]
    return Run(0, group, T, r, align), chains


def _level_specs(group: int, tmax: int):
    specs = []
    for align in ALIGNS:
        for r in (TAIL_ONE, TAIL_TWO) + TAILS_LOW_T:
            for T in range(1, tmax + 1):
                if r >= 56 and T < 2:
                    continue  # no such size
                if r in TAILS_LOW_T and T > 9:
                    continue
                specs.append((group, T, r, align))
    # edge runs behind the sweep (they do not disturb how its runs pair up):
    # the remaining tail edges, with the chains walking through every start
    # residue mod 16 (dword-aligned but not 16-byte aligned included)
    for T in (2, 9, 18):
        for r in (56, 63, TAIL_ONE):
            specs.append((group, T, r, WALK))
    return specs


def level_table(group: int, tmax: int = TMAX) -> list:
    """Runs of `group` equal-size chains, one run per T in 1..tmax, per tail form
    (r = 37 and r = 61, plus r = 0 and r = 55 for T <= 9) and per start
    alignment (0 and 5 mod 16), T ascending within each (tail, alignment).

    group = 64 returns two orderings, the second starting one run later, so a
    128-chain workgroup (pc4x2, pcx5) holds the runs (T, T+1) in one and
    (T+1, T+2) in the other.  group = 128 returns one table in which
    both 64-chain groups of such a workgroup have the same T."""
    if group not in (64, 128):
        raise ValueError("group is 64 or 128")
    specs = _level_specs(group, tmax)
    orders = [specs] if group == 128 else [specs, specs[1:] + specs[:1]]
    return [_pack(f"level{group}/{k}", [_level_run(*s) for s in order], 1000 + group + k)
            for k, order in enumerate(orders)]


def ragged_table() -> Table:
    """64-chain runs of 63 chains with T_long steps and one, at lane 37, with
    T_short: T_short in 1..20, T_long in {T_short + 1, T_short + 2, T_short + 7,
    26}.  Each run comes twice, one after the other (so a 128-chain workgroup
    holds both): all chains 16-byte aligned, then the short chain misaligned.
    The short chain's tail walks through the edge residues and its misaligned
    start through 1..15 mod 16."""
    specs = []
    k = 0
    for T_short in range(1, 21):
        for T_long in sorted({T_short + 1, T_short + 2, T_short + 7, TMAX}):
            r_long = (TAIL_ONE, TAIL_TWO)[k % 2]
            ok = [r for r in EDGE_TAILS if r < 56 or T_short >= 2]
            r_short = ok[k % len(ok)]
            for mis in (0, 1 + k % 15):
                chains = [(size_for(T_long, r_long), 0)] * 64
                chains[SHORT_LANE] = (size_for(T_short, r_short), mis)
                specs.append((Run(0, 64, T_long, r_long, 0, T_short, r_short, mis), chains))
            k += 1
    return _pack("ragged", specs, 2000)


def uniform_cases(tmax: int = TMAX) -> list:
    """(chunk_size, n, len, base_shift) for lbf_sha1_uniform_launch.

    For T in 1..tmax and both tail forms the chunk size 64 * (T - 1) + 37 or
    64 * (T - 2) + 61 is odd, so successive chunks start at every residue mod
    16; each comes with n = 64, 128 and 129 chunks, the last one `short` bytes
    long, short in {1, cs - 1, cs}, at base_shift 0 and 3 -- `short` and the
    shift rotate with the case number so that every (n, short, shift) occurs.
    The same again with the chunk size rounded up to a multiple of 16 (same T;
    every chunk aligned at shift 0, none at 3).  Three n = 65 cases carry the
    tail residues 55, 56 and 63."""
    cases = []
    k = 0
    for rounded in (False, True):
        for T in range(1, tmax + 1):
            for r in (TAIL_ONE, TAIL_TWO):
                if r >= 56 and T < 2:
                    continue
                cs = size_for(T, r)
                if rounded:
                    cs = (cs + 15) // 16 * 16
                    assert steps(cs) == T
                for n in (64, 128, 129):
                    short = (1, cs - 1, cs)[k % 3]
                    shift = (0, 3)[(k // 3) % 2]
                    cases.append((cs, n, (n - 1) * cs + short, shift))
                    k += 1
                k += 2  # 5 per (T, tail), coprime to the period 6: every n meets every (short, shift)
    for T, r, short, shift in ((9, 55, 1, 3), (10, 56, None, 0), (17, 63, None, 3)):
        cs = size_for(T, r)
        cases.append((cs, 65, 64 * cs + (short or cs), shift))
    return cases


def uniform_table(cs: int, n: int, length: int, first: int = 0):
    """Offsets (from the region's base) and sizes of chunks first..first+n-1."""
    offs = (np.arange(n, dtype=np.uint64) + np.uint64(first)) * np.uint64(cs)
    sizes = np.minimum(np.uint64(length) - offs, np.uint64(cs)).astype(np.uint32)
    return offs, sizes


# ---------------------------------------------------------------------------
# Model of the kernels' loop bounds, from the formulas above.
# ---------------------------------------------------------------------------
@dataclass
class Consumer:
    """One consumer wave: 64 table entries first..first+63 (live: below n)."""
    first: int
    live: int
    nsteps: int       # block steps (barriers) of its workgroup
    min_steps: int    # steps every live chain of its 64 has
    fast_end: int

    def fast_trips(self, U: int) -> int:
        return self.fast_end // U


def loop_model(totals, per_wg: int) -> list:
    """The consumers of a launch over chains with `totals` steps each, 64 (pc4)
    or 128 (pc4x2, pcx5: two consumers, one per 64) chains to a workgroup.
    nsteps is the maximum over the workgroup, min_steps the minimum over the
    consumer's own live chains, fast_end = min(min_steps, nsteps - 1).  A
    consumer with no live chain (the second of a last workgroup with <= 64
    chains) hashes nothing that is kept and is left out."""
    if per_wg not in (64, 128):
        raise ValueError("64 or 128 chains per workgroup")
    t = np.asarray(totals, dtype=np.int64)
    out = []
    for w0 in range(0, t.size, per_wg):
        nsteps = int(t[w0:w0 + per_wg].max())
        for g0 in range(w0, min(w0 + per_wg, t.size), 64):
            mine = t[g0:g0 + 64]
            min_steps = int(mine.min())
            out.append(Consumer(g0, int(mine.size), nsteps, min_steps, min(min_steps, nsteps - 1) if nsteps else 0))
    return out

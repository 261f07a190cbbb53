"""Layouts past byte 2^32 and past 65,536 entries -- TEST INFRASTRUCTURE.

Pure numpy, no GPU.  tests/test_gpu_large_index.py launches these layouts on
the device entry points (lbf_sha1_launch, lbf_sha1_uniform_launch,
lbf_sha1_update_launch, lbf_b64_update_launch) and the host batch calls;
tests/test_large_index.py asserts that they reach what they are built to reach.

Every large buffer is one allocation that starts at offset 0 and ends past the
highest offset used.  Only two windows of it ever hold data:

    the high window    [lo, hi), lo < 2^32 < hi
    the alias window   [0, hi - 2^32): the high window's positions past the
                       line, minus 2^32

A kernel that keeps an offset (or a sum of offset and index) in 32 bits lands in
the alias window, inside the same allocation: it computes a wrong result and
cannot fault.  For reads the alias window holds other bytes than the high one;
for writes it holds the fill value, which the GPU test then finds unchanged.
Nothing uploads or downloads a whole 4 GiB buffer: `uploads()` yields the
(offset, bytes) pairs and the tests read the two windows back.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass

import numpy as np

LINE = 1 << 32
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "bitflood_amd", "csrc")
ABOVE_PHASES = (1, 5, 15, 8)         # start residues mod 16 above the line; 8 for the 16-byte load path
STATE_BYTES = 96
S = -(-LINE // STATE_BYTES)          # the first record that lies wholly at or past byte 2^32 of a state array
STATE_INDICES = (S - 2, S - 1, S, S + 1, S + 40)   # below, across, and three above byte 2^32
STATE_NEIGHBOUR = S + 2
N_STATES = S + 64
BELOW, STRADDLE, AT, ABOVE = "below", "straddle", "at", "above"


def kind_of(start: int, size: int) -> str:
    """Where the byte range [start, start + size) lies against the line."""
    if start == LINE:
        return AT
    if start > LINE:
        return ABOVE
    return STRADDLE if start + size > LINE else BELOW


def place(sizes, phases, anchor: int, mode: str) -> np.ndarray:
    """Starts of disjoint ranges laid in order around the line: entry k is
    `sizes[k]` bytes at a start that is phases[k] mod 16.  Entry `anchor` starts
    exactly at 2^32 (mode AT; its phase must be 0) or has byte 2^32 inside it,
    near its middle (mode STRADDLE; it must be longer than 64 bytes).  The
    entries before it lie below the line, the ones after it above."""
    n = len(sizes)
    starts = [0] * n
    size, phase = int(sizes[anchor]), int(phases[anchor])
    if mode == AT:
        if phase != 0:
            raise ValueError("an entry at 2^32 has phase 0")
        starts[anchor] = LINE
    elif mode == STRADDLE:
        if size <= 64:
            raise ValueError("a straddling entry is longer than 64 bytes")
        starts[anchor] = (LINE - size // 2) // 16 * 16 + phase - 16
    else:
        raise ValueError(mode)
    pos = starts[anchor] + size
    for k in range(anchor + 1, n):
        starts[k] = (pos + 15 - int(phases[k])) // 16 * 16 + int(phases[k])
        pos = starts[k] + int(sizes[k])
    nxt = starts[anchor]
    for k in range(anchor - 1, -1, -1):
        starts[k] = (nxt - int(sizes[k]) - int(phases[k])) // 16 * 16 + int(phases[k])
        nxt = starts[k]
    return np.array(starts, dtype=np.uint64)


@dataclass
class Ranges:
    """Byte ranges of one large buffer with the two windows that hold data.
    `window` are the bytes of [lo, lo + window.size), `alias` those of
    [0, alias.size); `alloc` is the size of the allocation."""
    offsets: np.ndarray       # uint64, true offsets from the buffer's start
    sizes: np.ndarray         # uint32
    lo: int
    window: np.ndarray
    alias: np.ndarray
    alloc: int

    @property
    def n(self) -> int:
        return int(self.offsets.size)

    @property
    def hi(self) -> int:
        return self.lo + int(self.window.size)

    def kinds(self) -> list:
        return [kind_of(int(o), int(s)) for o, s in zip(self.offsets, self.sizes)]

    def rel(self) -> np.ndarray:
        """The offsets from the high window's start: what a CPU reference of
        `window` takes."""
        return self.offsets - np.uint64(self.lo)

    def true_bytes(self, i: int) -> bytes:
        a = int(self.offsets[i]) - self.lo
        return self.window[a:a + int(self.sizes[i])].tobytes()

    def truncated_bytes(self, i: int) -> bytes:
        """What entry i reads when every byte position is taken mod 2^32."""
        o, s = int(self.offsets[i]), int(self.sizes[i])
        out = bytearray()
        for p in range(o, o + s):
            out.append(int(self.alias[p - LINE]) if p >= LINE else int(self.window[p - self.lo]))
        return bytes(out)

    def uploads(self):
        """(offset, bytes) pairs: the alias window first, then the high one."""
        yield 0, self.alias
        yield self.lo, self.window


def windows(offsets, sizes, seed: int, margin: int = 64, fill=None) -> Ranges:
    """The two windows around `offsets`/`sizes`: seeded bytes for reads, or
    `fill` everywhere for writes.  The windows reach `margin` bytes past the
    outermost ranges, so guard bytes around them can be read back too."""
    offsets = np.asarray(offsets, dtype=np.uint64)
    sizes = np.asarray(sizes, dtype=np.uint32)
    ends = offsets.astype(np.int64) + sizes
    lo = int(offsets.min()) // 16 * 16 - margin
    hi = (int(ends.max()) + 15) // 16 * 16 + margin
    if not lo < LINE < hi:
        raise ValueError("the ranges do not reach across 2^32")
    if fill is None:
        rng = np.random.default_rng(seed)
        window = rng.integers(0, 256, hi - lo, dtype=np.uint8)
        alias = rng.integers(0, 256, hi - LINE, dtype=np.uint8)
    else:
        window = np.full(hi - lo, fill, dtype=np.uint8)
        alias = np.full(hi - LINE, fill, dtype=np.uint8)
    return Ranges(offsets, sizes, lo, window, alias, hi)


def _phases(n: int, anchor: int) -> list:
    """Below the anchor every residue in turn; above it ABOVE_PHASES first."""
    ph = [(3 * k) % 16 for k in range(n)]
    for j, k in enumerate(range(anchor + 1, n)):
        ph[k] = (ABOVE_PHASES + (0, 4, 12))[j % 7]
    ph[anchor] = 0
    return ph


def table_case(n: int = 200, seed: int = 11) -> Ranges:
    """lbf_sha1_launch / lbf_sha1_update_launch: n ranges of 0..3,000 bytes, both
    SHA-1 tail forms and the block edges among them.  Two thirds are laid
    disjoint around an entry that starts at 2^32; the last third overlaps them
    (reads may), laid around an entry that straddles the line, and four more
    straddle it by 1, 7, 16 and 63 bytes.  The order is shuffled, so one wave
    mixes entries below and above the line."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, 3001, n).tolist()
    for k, s in enumerate((0, 1, 55, 56, 63, 64, 119, 120, 127, 128, 2999, 3000)):
        sizes[(k * 17) % n] = s
    n1 = 2 * n // 3
    a1, a2 = n1 // 2, (n - n1) // 2
    sizes[a1] = 777
    sizes[n1 + a2] = 1501
    s1 = place(sizes[:n1], _phases(n1, a1), a1, AT)
    s2 = place(sizes[n1:], _phases(n - n1, a2), a2, STRADDLE)
    extra_sizes = [200, 61, 1000, 64]
    extra = [LINE - 1, LINE - 7, LINE - 16, LINE - 63]
    offsets = np.concatenate([s1, s2, np.array(extra, dtype=np.uint64)])
    sizes = np.array(sizes + extra_sizes, dtype=np.uint32)
    order = rng.permutation(offsets.size)
    return windows(offsets[order], sizes[order], seed + 1)


def uniform_cases() -> list:
    """(chunk_size, first_chunk, n, len) for lbf_sha1_uniform_launch, the region
    starting at the buffer's start: first_chunk * chunk_size < 2^32 <
    (first_chunk + n) * chunk_size, n covers two 128-chain workgroups and a
    partial wave, and the last chunk is short.  One chunk size is odd, so the
    chunks start at every residue mod 16; the other divides 2^32, so chunk
    2^32 / chunk_size starts exactly at the line."""
    cases = []
    for cs, n, before, short in ((613, 170, 83, 41), (1024, 150, 70, 1000)):
        first = LINE // cs - before
        cases.append((cs, first, n, (first + n - 1) * cs + short))
    return cases


def uniform_ranges(cs: int, first: int, n: int, length: int, seed: int = 21) -> Ranges:
    offs = (np.arange(n, dtype=np.uint64) + np.uint64(first)) * np.uint64(cs)
    sizes = np.minimum(np.uint64(length) - offs, np.uint64(cs)).astype(np.uint32)
    r = windows(offs, sizes, seed + cs, margin=0)
    assert r.lo <= int(offs[0]) and r.hi >= length
    return r


def thinned(firsts, seconds) -> list:
    """Every other (first piece, second piece) size pair, as the black squares
    of a chessboard (every size of both lists stays in), and four more."""
    combos = [(a, b) for i, a in enumerate(firsts) for j, b in enumerate(seconds) if (i + j) % 2 == 0]
    return combos + [(64, 200), (63, 129), (1, 65), (56, 128)]


def piece_cases(firsts, seconds, seed: int = 31):
    """lbf_sha1_update_launch: chains fed in two launches.  Chain k's first
    piece is firsts[k] bytes, its second seconds[k]; each launch's pieces lie
    disjoint around the line at the phases 0, 1, 8 and 15 mod 16, the first
    launch's around a piece that starts at 2^32, the second's around one that
    straddles it.  Both launches read one window, so the launches' pieces
    overlap one another."""
    n = len(firsts)
    assert n == len(seconds)
    a1 = next(k for k in range(n // 3, n) if k % 4 == 0)           # phase 0
    a2 = next(k for k in range(n // 2, n) if seconds[k] > 64)
    ph = [(0, 1, 8, 15)[k % 4] for k in range(n)]
    o1 = place(firsts, ph, a1, AT)
    o2 = place(seconds, ph, a2, STRADDLE)
    both = windows(np.concatenate([o1, o2]), np.concatenate([firsts, seconds]), seed)
    first = Ranges(o1, np.asarray(firsts, dtype=np.uint32), both.lo, both.window, both.alias, both.alloc)
    second = Ranges(o2, np.asarray(seconds, dtype=np.uint32), both.lo, both.window, both.alias, both.alloc)
    return first, second


def slot_case(caps, anchor: int, mode: str, fill: int) -> Ranges:
    """Output slots of caps[k] bytes, disjoint, around the line: slot `anchor`
    starts at 2^32 or straddles it; the slots above it start at the phases 0,
    5 and 15 mod 16 in turn, the ones below at every residue.  Both windows
    hold `fill`."""
    n = len(caps)
    ph = [(5 * k + 3) % 16 for k in range(n)]
    for j, k in enumerate(range(anchor + 1, n)):
        ph[k] = (0, 5, 15)[j % 3]
    ph[anchor] = 0 if mode == AT else 11
    return windows(place(caps, ph, anchor, mode), caps, 0, fill=fill)


def text_case(lens, anchor: int, mode: str, phase: int, seed: int) -> Ranges:
    """Text pieces of lens[k] characters, disjoint, around the line, each at
    `phase` mod 16 (the anchor of mode AT at 0).  The windows are seeded
    alphabet characters; the caller writes its pieces into `window`."""
    ph = [phase] * len(lens)
    if mode == AT:
        ph[anchor] = 0
    r = windows(place(lens, ph, anchor, mode), lens, seed)
    alphabet = np.frombuffer(b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/", dtype=np.uint8)
    r.window = alphabet[r.window & 63]
    r.alias = alphabet[r.alias & 63]
    return r


# ---------------------------------------------------------------------------
# More than 65,536 entries: the constants come from the sources, so that a
# launcher that changes its geometry fails tests/test_large_index.py instead of
# leaving the GPU tests with nothing to pin.
# ---------------------------------------------------------------------------
def _source(name: str) -> str:
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


_GEOMETRY = r"const uint32_t threads = p\.n <= (\d+)u \? (\d+)u : (\d+)u;"


def launch_geometry() -> dict:
    """{launcher: (entry threshold, threads at or below it, threads above it)}
    of launch_lane (sha1_kernels.hip) and lbf_sha1_update_launch
    (sha1_update.hip), and the block size of b64_length_kernel (b64_update.hip)."""
    out = {}
    for key, name in (("lane", "sha1_kernels.hip"), ("update", "sha1_update.hip")):
        found = re.findall(_GEOMETRY, _source(name))
        if len(found) != 1:
            raise AssertionError(f"{name}: {len(found)} workgroup-size switches, expected one")
        out[key] = tuple(int(x) for x in found[0])
    b64 = _source("b64_update.hip")
    bounds = re.search(r"__launch_bounds__\((\d+)\) b64_length_kernel", b64)
    grid = re.search(r"lbf::b64_length_kernel, dim3\(\(\(uint32_t\)n \+ (\d+)u\) / (\d+)u\), dim3\((\d+)\)", b64)
    if not bounds or not grid:
        raise AssertionError("b64_update.hip: b64_length_kernel's launch not found")
    out["length"] = (int(bounds.group(1)),) + tuple(int(x) for x in grid.groups())
    return out


def entry_count() -> int:
    """The entry threshold + a full 64-lane wave + a ragged one of 37."""
    g = launch_geometry()
    assert g["lane"][0] == g["update"][0]
    return g["lane"][0] + 64 + 37


def small_table(n: int, seed: int, top: int = 200):
    """n chains of 0..top bytes packed at unaligned starts: (data, offsets, sizes)."""
    rng = np.random.default_rng(seed)
    sizes = rng.integers(0, top + 1, n).astype(np.uint32)
    gaps = rng.integers(0, 4, n)
    offs = np.cumsum(sizes.astype(np.int64) + gaps) - sizes + 1
    data = rng.integers(0, 256, int(offs[-1]) + int(sizes[-1]) + 16, dtype=np.uint8)
    return data, offs.astype(np.uint64), sizes

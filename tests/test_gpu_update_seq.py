"""Several pieces of one chain absorbed in one call, in order, on the GPU:
lbf_sha1_update_seq_launch (one lane per chain, the record's header in
registers from the chain's first piece to its last) and
lbf_sha1_update_seq_batch / ChunkHasher.update_chunks_seq.

Expected values come from hashlib and, for records in mid-chain,
tests/sha1_model.py -- never from a GPU path; the launch and the batch call are
run on the same chains and held to the same expectations.  Arenas of outputs
are pre-filled with 0xEE, so what a call must leave alone can be asserted.
Shapes are the smallest at which the kernel can go wrong: every size around
the 64-byte block and the 56-byte padding edge in several orders, every source
phase of the 16-byte load path, ragged waves, and the 256-thread launch shape.
"""
import hashlib

import numpy as np
import pytest

from bitflood_amd import (STATE_DTYPE, DeviceBuffer, LbfError, _capi, chain_table, new_b64_states,
                          new_states)
from bitflood_amd import hashing as H
from tests import sha1_model
from tests import wire_piece_model as M

pytestmark = pytest.mark.gpu

FILL = 0xEE
SIZES = [0, 1, 9, 55, 56, 63, 64, 65, 127, 128, 129, 1000]


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


class Arena:
    """Pieces laid out in one buffer: each at `phase` mod 16, or (phase None)
    one right behind the other."""

    def __init__(self, phase=None):
        self.phase, self.parts, self.len = phase, [], 0

    def put(self, data: bytes) -> int:
        pad = 0 if self.phase is None else (self.phase - self.len) % 16
        self.parts.append(bytes(pad) + bytes(data))
        off = self.len + pad
        self.len = off + len(data)
        return off

    def buffer(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.parts) + b"\0", dtype=np.uint8).copy()


def expectation(chains, start=None):
    """chains: [(state index, [(bytes, final), ...])].  Per chain the digest of
    every final piece (None for the others) and the chain's sha1_model state
    behind its last piece, continued from start[state] (a sha1_model state) or
    from the initial value."""
    digests, states = [], {}
    for s, pieces in chains:
        st = (start or {}).get(s, sha1_model.init())
        pending, row = b"", []
        for data, fin in pieces:
            pending += bytes(data)
            if fin:  # hashlib where the chunk began in this call, the model where it continues a record
                row.append(sha1(pending) if st == sha1_model.init() else
                           sha1_model.final(sha1_model.update(st, pending)))
                st, pending = sha1_model.init(), b""
            else:
                row.append(None)
        states[s] = sha1_model.update(st, pending)
        digests.append(row)
    return digests, states


def check_states(got, n_states, want_states, before):
    """Touched states equal the model's records (a state whose chain ended is
    byte for byte a fresh one); every other state is byte for byte as before."""
    idx = sorted(want_states)
    want = M.sha_records([want_states[s] for s in idx], STATE_DTYPE)
    assert M.sha_records_differ(got[idx], want) == [], [idx[k] for k in M.sha_records_differ(got[idx], want)]
    fresh = new_states(1).tobytes()
    for s in idx:
        if want_states[s] == sha1_model.init():
            assert got[s].tobytes() == fresh, s
    rest = np.setdiff1d(np.arange(n_states), idx)
    assert got[rest].tobytes() == before[rest].tobytes()


def run_launch(chains, n_states, phase=None, states=None, start=None, stream=None):
    """The chains through ONE lbf_sha1_update_seq_launch, pieces in table order
    (chain after chain); every final piece gets an expected digest, every third
    of them a wrong one.  Everything is checked; returns the states."""
    before = new_states(n_states) if states is None else states.copy()
    arena = Arena(phase)
    offs, sizes, fin, first = [], [], [], [0]
    for _, pieces in chains:
        for data, f in pieces:
            offs.append(arena.put(data))
            sizes.append(len(data))
            fin.append(1 if f else 0)
        first.append(len(offs))
    n = len(offs)
    buf = arena.buffer()
    want_dig, want_states = expectation(chains, start)
    flat = [d for row in want_dig for d in row]
    expected = np.zeros((max(n, 1), 20), dtype=np.uint8)
    nth = 0
    wrong = set()
    for i, d in enumerate(flat):
        if d is not None:
            expected[i] = np.frombuffer(d, dtype=np.uint8)
            if nth % 3 == 2:
                expected[i, 5] ^= 0x04
                wrong.add(i)
            nth += 1
    bufs = {k: DeviceBuffer(max(b, 16)) for k, b in dict(st=96 * n_states, cs=4 * len(chains), cf=4 * len(first),
                                                         data=buf.size, off=8 * n, size=4 * n, fin=n, dig=20 * n,
                                                         exp=20 * n, ver=n).items()}
    try:
        bufs["st"].upload(before)
        bufs["cs"].upload(np.array([s for s, _ in chains], dtype=np.uint32))
        bufs["cf"].upload(np.array(first, dtype=np.uint32))
        bufs["data"].upload(buf)
        bufs["off"].upload(np.array(offs, dtype=np.uint64))
        bufs["size"].upload(np.array(sizes, dtype=np.uint32))
        bufs["fin"].upload(np.array(fin, dtype=np.uint8))
        bufs["dig"].upload(np.full(max(20 * n, 16), FILL, dtype=np.uint8))
        bufs["ver"].upload(np.full(max(n, 16), FILL, dtype=np.uint8))
        bufs["exp"].upload(expected)
        H.update_seq_launch(bufs["st"], n_states, bufs["cs"], bufs["cf"], len(chains), bufs["data"], bufs["off"],
                            bufs["size"], bufs["fin"], n, bufs["dig"], bufs["exp"], bufs["ver"], stream=stream)
        H.synchronize()
        got = bufs["st"].download(96 * n_states).view(STATE_DTYPE)
        dig = bufs["dig"].download(20 * n).reshape(n, 20)
        ver = bufs["ver"].download(n)
    finally:
        for b in bufs.values():
            b.free()
    for i, d in enumerate(flat):
        if d is None:  # entries of pieces that are not final are left alone
            assert (dig[i] == FILL).all() and ver[i] == FILL, i
        else:
            assert dig[i].tobytes() == d, (i, sizes[i])
            assert ver[i] == (0 if i in wrong else 1), i
    check_states(got, n_states, want_states, before)
    return got


def interleaved(chains):
    """The chains' pieces in a caller's order: piece r of every chain that has
    one, round by round.  Returns [(chain, piece)]."""
    rounds = max((len(p) for _, p in chains), default=0)
    return [(c, r) for r in range(rounds) for c, (_, p) in enumerate(chains) if r < len(p)]


def raw_batch(hasher, fn, states, buf, offs, sizes, state_of, final, dig, expected, ver):
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    so = None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32)
    fin = None if final is None else np.ascontiguousarray(final, dtype=np.uint8)
    return getattr(_capi.load(), fn)(hasher._h, states.ctypes.data, states.size, p(so), buf.ctypes.data, buf.size,
                                     offs.ctypes.data, sizes.ctypes.data, p(fin), offs.size, p(dig), p(expected),
                                     p(ver))


def run_batch(hasher, chains, n_states, phase=None, states=None, start=None):
    """The same chains through ONE lbf_sha1_update_seq_batch, pieces interleaved
    round by round, with the caller's own output arrays."""
    before = new_states(n_states) if states is None else states.copy()
    got = before.copy()
    order = interleaved(chains)
    arena = Arena(phase)
    offs = [arena.put(chains[c][1][r][0]) for c, r in order]
    buf = arena.buffer()
    n = len(order)
    want_dig, want_states = expectation(chains, start)
    dig = np.full((n, 20), FILL, dtype=np.uint8)
    ver = np.full(n, FILL, dtype=np.uint8)
    expected = np.zeros((n, 20), dtype=np.uint8)
    for i, (c, r) in enumerate(order):
        if want_dig[c][r] is not None:
            expected[i] = np.frombuffer(want_dig[c][r], dtype=np.uint8)
            expected[i, 0] ^= (i % 2)  # every other one is wrong
    rc = raw_batch(hasher, "lbf_sha1_update_seq_batch", got, buf, offs, [len(chains[c][1][r][0]) for c, r in order],
                   [chains[c][0] for c, _ in order], [chains[c][1][r][1] for c, r in order], dig, expected, ver)
    assert rc == 0, _capi.load().lbf_last_error().decode()
    for i, (c, r) in enumerate(order):
        if want_dig[c][r] is None:
            assert (dig[i] == FILL).all() and ver[i] == FILL, i
        else:
            assert dig[i].tobytes() == want_dig[c][r], (i, c, r)
            assert ver[i] == (0 if i % 2 else 1), i
    check_states(got, n_states, want_states, before)
    return got


def both(hasher, chains, n_states, phase=None):
    a = run_launch(chains, n_states, phase)
    b = run_batch(hasher, chains, n_states, phase)
    # the two agree on every state, the block's bytes past `buffered` left out
    assert M.sha_records_differ(a, b) == [] and M.sha_records_differ(b, a) == []


def rnd(rng, n) -> bytes:
    return rng.integers(0, 256, int(n), dtype=np.uint8).tobytes()


@pytest.mark.parametrize("final", [True, False])
def test_sizes_around_the_block_in_several_orders(hasher, final):
    """One chain per order of SIZES (as listed, reversed, rotated, shuffled):
    every size meets several `buffered` values.  With `final` the last piece
    ends the chain; without, the records are the model's."""
    rng = np.random.default_rng(1)
    orders = [SIZES, SIZES[::-1], SIZES[5:] + SIZES[:5]] + [list(rng.permutation(SIZES)) for _ in range(5)]
    chains = []
    for k, order in enumerate(orders):
        pieces = [(rnd(rng, s), False) for s in order]
        if final:
            pieces[-1] = (pieces[-1][0], True)
        chains.append((2 * k + 1, pieces))  # odd states: the even ones stay untouched
    both(hasher, chains, 2 * len(orders) + 1, phase=3)


def test_small_pieces_exact_blocks_and_an_empty_final(hasher):
    rng = np.random.default_rng(2)
    chains = [
        (0, [(rnd(rng, 10), False)] * 3),                                     # the block never fills
        (1, [(rnd(rng, 10), False), (rnd(rng, 10), False), (rnd(rng, 10), True)]),
        (2, [(rnd(rng, 10), False), (rnd(rng, 54), False), (rnd(rng, 64), False), (rnd(rng, 30), False),
             (rnd(rng, 34), False)]),                                         # every piece ends on a block edge
        (3, [(rnd(rng, 64), False), (rnd(rng, 128), False), (rnd(rng, 1), False), (rnd(rng, 63), True)]),
        (4, [(rnd(rng, 70), False), (b"", True)]),                            # a final piece of size 0
        (5, [(b"", False), (b"", False), (b"", True)]),                       # the empty chunk
        (6, [(b"", True)]),
        (7, [(rnd(rng, 55), False), (b"", False), (rnd(rng, 1), True)]),      # the padding edge
        (8, [(rnd(rng, 56), False), (b"", True)]),
    ]
    both(hasher, chains, 9, phase=None)


@pytest.mark.parametrize("contiguous", [True, False])
def test_every_source_phase(hasher, contiguous):
    """Pieces at every offset mod 16 (the aligned two-blocks-in-flight loop runs
    only where a piece's full blocks start on a 16-byte edge -- decided piece by
    piece), scattered with gaps or one right behind the other."""
    rng = np.random.default_rng(3)
    sizes = [200, 7, 64, 129, 16, 300]
    if contiguous:
        chains = [(k, [(rnd(rng, s + k), k % 2 == 0 and j == len(sizes) - 1) for j, s in enumerate(sizes)])
                  for k in range(16)]  # the sizes shift the phase from piece to piece
        both(hasher, chains, 16, phase=None)
    else:
        for phase in range(16):
            chains = [(0, [(rnd(rng, s), False) for s in sizes]), (1, [(rnd(rng, s), j == 5) for j, s in
                                                                       enumerate(sizes)])]
            run_launch(chains, 2, phase=phase)
        both(hasher, chains, 2, phase=11)


def test_ragged_chains_over_two_waves(hasher):
    """65 chains of 0..7 pieces: two waves, an empty chain in the middle,
    ragged piece counts within a wave; half the chains end."""
    rng = np.random.default_rng(4)
    chains = []
    for c in range(65):
        count = 0 if c == 32 else int(rng.integers(0, 8))
        pieces = [(rnd(rng, rng.integers(0, 300)), False) for _ in range(count)]
        if count and c % 2:
            pieces[-1] = (pieces[-1][0], True)
        chains.append((64 - c, pieces))  # states in reverse
    before = new_states(65)
    got = run_launch(chains, 65, phase=5)
    empty = [s for s, p in chains if not p]
    assert 32 in empty and got[empty].tobytes() == before[empty].tobytes()
    run_batch(hasher, [ch for ch in chains if ch[1]], 65, phase=5)


def test_the_256_thread_launch_shape(hasher):
    """65,537 chains of one or two pieces of at most 64 bytes, all ending: past
    65,536 chains the launch uses 256-thread workgroups."""
    rng = np.random.default_rng(5)
    n_chains = 65537
    two = rng.integers(0, 2, n_chains).astype(bool)
    sizes = rng.integers(0, 65, (n_chains, 2))
    data = rng.integers(0, 256, int(sizes.sum()) + 64, dtype=np.uint8)
    counts = 1 + two.astype(np.int64)
    first = np.zeros(n_chains + 1, dtype=np.uint32)
    first[1:] = np.cumsum(counts)
    n = int(first[-1])
    piece_size = np.zeros(n, dtype=np.uint32)
    piece_size[first[:-1]] = sizes[:, 0]
    piece_size[first[:-1][two] + 1] = sizes[two, 1]
    offs = np.zeros(n, dtype=np.uint64)
    offs[1:] = np.cumsum(piece_size[:-1])
    fin = np.zeros(n, dtype=np.uint8)
    fin[first[1:] - 1] = 1
    raw = data.tobytes()
    want = np.full((n, 20), FILL, dtype=np.uint8)
    for c in range(n_chains):
        lo, hi = int(offs[first[c]]), int(offs[first[c + 1] - 1]) + int(piece_size[first[c + 1] - 1])
        want[first[c + 1] - 1] = np.frombuffer(sha1(raw[lo:hi]), dtype=np.uint8)
    bufs = {k: DeviceBuffer(b) for k, b in dict(st=96 * n_chains, cf=4 * (n_chains + 1), data=data.size, off=8 * n,
                                                size=4 * n, fin=n, dig=20 * n).items()}
    try:
        bufs["st"].upload(new_states(n_chains))
        bufs["cf"].upload(first)
        bufs["data"].upload(data)
        bufs["off"].upload(offs)
        bufs["size"].upload(piece_size)
        bufs["fin"].upload(fin)
        bufs["dig"].upload(np.full(20 * n, FILL, dtype=np.uint8))
        # chain c continues state c: no chain_state array
        H.update_seq_launch(bufs["st"], n_chains, None, bufs["cf"], n_chains, bufs["data"], bufs["off"], bufs["size"],
                            bufs["fin"], n, bufs["dig"])
        H.synchronize()
        dig = bufs["dig"].download(20 * n).reshape(n, 20)
        states = bufs["st"].download(96 * n_chains)
    finally:
        for b in bufs.values():
            b.free()
    bad = np.flatnonzero((dig != want).any(axis=1))
    assert bad.size == 0, bad[:8].tolist()
    assert states.tobytes() == new_states(n_chains).tobytes()


def test_a_final_in_mid_run_starts_the_next_chunk(hasher):
    """Launch only (the batch call refuses it): a final piece that is not its
    chain's last ends the chunk and writes its outputs, and the pieces behind
    it begin a new chunk -- both digests are right and the record afterwards is
    the second chunk's, what successive launches give."""
    rng = np.random.default_rng(6)
    chains = [
        (1, [(rnd(rng, 100), False), (rnd(rng, 30), True), (rnd(rng, 70), False), (rnd(rng, 5), False)]),
        (0, [(rnd(rng, 64), True), (rnd(rng, 64), True), (b"", True), (rnd(rng, 200), True)]),
        (2, [(rnd(rng, 9), True), (rnd(rng, 3), False)]),
    ]
    got = run_launch(chains, 3, phase=7)
    assert got["total"].tolist() == [0, 75, 3] and got["buffered"].tolist() == [0, 11, 3]
    # the second chunk's record goes on through the call that takes one piece per state
    tail = rnd(rng, 77)
    out = hasher.update_chunks(got, np.frombuffer(tail, dtype=np.uint8), [0], [77], state_of=[1], final=[1])
    assert out[0].tobytes() == sha1(chains[0][1][2][0] + chains[0][1][3][0] + tail)
    # the batch call refuses the same table, everything untouched
    st = new_states(3)
    buf = np.zeros(64, dtype=np.uint8)
    dig = np.full((3, 20), FILL, dtype=np.uint8)
    rc = raw_batch(hasher, "lbf_sha1_update_seq_batch", st, buf, [0, 0, 0], [4, 4, 4], [2, 0, 2], [1, 1, 0], dig, None,
                   None)
    msg = _capi.load().lbf_last_error().decode()
    assert rc == _capi.LBF_ERR_INVALID and "piece 0" in msg and "is final" in msg, msg
    assert st.tobytes() == new_states(3).tobytes() and (dig == FILL).all()


def test_a_forged_table_touches_nothing_it_should_not():
    """A chain whose state index is out of range is skipped whole; chain_first
    entries past n are clamped and an inverted range is empty; pieces that no
    chain names are left alone -- states, digests and verdicts keep their
    bytes, and the honest chains beside them are exact."""
    rng = np.random.default_rng(7)
    n_states, n = 4, 8
    data = [rnd(rng, s) for s in (70, 5, 64, 1, 100, 33, 12, 90)]
    arena = Arena(2)
    offs = [arena.put(d) for d in data]
    buf = arena.buffer()
    # chain 0: state 1, pieces [0, 2); chain 1: state 9 (no such state), pieces [2, 4): skipped whole; chain 2:
    # state 2, [4, 4): no piece; chain 3: state 0, [4, 1000): clamped to [4, 8)
    chain_state = np.array([1, 9, 2, 0], dtype=np.uint32)
    chain_first = np.array([0, 2, 4, 4, 1000], dtype=np.uint32)
    fin = np.array([0, 1, 1, 1, 0, 0, 0, 1], dtype=np.uint8)
    before = new_states(n_states)
    before["block"][:] = 0x5A  # whatever lies in a fresh record's block stays where nothing is written
    bufs = {k: DeviceBuffer(b) for k, b in dict(st=96 * n_states, cs=16, cf=20, data=buf.size, off=8 * n, size=4 * n,
                                                fin=n, dig=20 * n).items()}
    try:
        def launch(first, states, n_chains=4):
            bufs["st"].upload(states)
            bufs["cs"].upload(chain_state)
            bufs["cf"].upload(first)
            bufs["data"].upload(buf)
            bufs["off"].upload(np.array(offs, dtype=np.uint64))
            bufs["size"].upload(np.array([len(d) for d in data], dtype=np.uint32))
            bufs["fin"].upload(fin)
            bufs["dig"].upload(np.full(20 * n, FILL, dtype=np.uint8))
            H.update_seq_launch(bufs["st"], n_states, bufs["cs"], bufs["cf"], n_chains, bufs["data"], bufs["off"],
                                bufs["size"], bufs["fin"], n, bufs["dig"])
            H.synchronize()
            return bufs["st"].download(96 * n_states).view(STATE_DTYPE), bufs["dig"].download(20 * n).reshape(n, 20)

        got, dig = launch(chain_first, before)
        assert dig[1].tobytes() == sha1(data[0] + data[1])
        assert dig[7].tobytes() == sha1(data[4] + data[5] + data[6] + data[7])  # [4, 1000) clamped to [4, 8)
        for i in (0, 2, 3, 4, 5, 6):
            assert (dig[i] == FILL).all(), i  # not final, or the skipped chain's
        assert got[[2, 3]].tobytes() == before[[2, 3]].tobytes()  # the empty chain's state, and one nobody names
        assert got[0]["total"] == 0 and got[1]["total"] == 0 and got[0]["buffered"] == 0
        # three chains only: pieces 4 .. 7 are no chain's, and state 0 is nobody's
        got, dig = launch(chain_first, before, n_chains=3)
        assert dig[1].tobytes() == sha1(data[0] + data[1]) and (dig[[0, 2, 3, 4, 5, 6, 7]] == FILL).all()
        assert got[[0, 2, 3]].tobytes() == before[[0, 2, 3]].tobytes()
        # an inverted range, and a first entry past n: both empty
        got, dig = launch(np.array([6, 2, 4, 4, 4], dtype=np.uint32), before)  # chain 0 = [6, 2)
        assert got.tobytes() == before.tobytes() and (dig == FILL).all()
        got, dig = launch(np.array([1000, 2000, 4, 4, 4], dtype=np.uint32), before)
        assert got.tobytes() == before.tobytes() and (dig == FILL).all()
        # the checks before the launch: a table that does not fit its allocation, a misaligned one
        with pytest.raises(LbfError) as e:
            H.update_seq_launch(bufs["st"], n_states, bufs["cs"], bufs["cf"], 5, bufs["data"], bufs["off"],
                                bufs["size"], bufs["fin"], n, bufs["dig"])
        assert e.value.status == _capi.LBF_ERR_INVALID and "chain_" in str(e.value), str(e.value)
        with pytest.raises(LbfError) as e:
            H.update_seq_launch(bufs["st"], n_states, bufs["cs"], bufs["cf"].ptr + 2, 3, bufs["data"], bufs["off"],
                                bufs["size"], bufs["fin"], n, bufs["dig"])
        assert e.value.status == _capi.LBF_ERR_INVALID and "aligned" in str(e.value), str(e.value)
        with pytest.raises(LbfError) as e:
            H.update_seq_launch(bufs["st"], n_states, bufs["cs"], None, 4, bufs["data"], bufs["off"], bufs["size"],
                                bufs["fin"], n, bufs["dig"])
        assert e.value.status == _capi.LBF_ERR_INVALID
    finally:
        for b in bufs.values():
            b.free()


def test_a_call_without_repeats_equals_update_chunks(hasher):
    rng = np.random.default_rng(8)
    n_states, n = 40, 25
    pre = [rnd(rng, rng.integers(0, 200)) for _ in range(n_states)]
    piece = [rnd(rng, rng.integers(0, 700)) for _ in range(n)]
    arena = Arena(5)
    pre_off = [arena.put(p) for p in pre]
    off = [arena.put(p) for p in piece]
    buf = arena.buffer()
    subset = rng.permutation(n_states)[:n]
    final = (np.arange(n) % 2).astype(np.uint8)
    states = new_states(n_states)
    hasher.update_chunks(states, buf, pre_off, [len(p) for p in pre])
    results = []
    for fn in ("lbf_sha1_update_batch", "lbf_sha1_update_seq_batch"):
        st = states.copy()
        dig = np.full((n, 20), FILL, dtype=np.uint8)
        ver = np.full(n, FILL, dtype=np.uint8)
        exp = np.zeros((n, 20), dtype=np.uint8)
        assert raw_batch(hasher, fn, st, buf, off, [len(p) for p in piece], subset, final, dig, exp, ver) == 0
        results.append((st.tobytes(), dig.tobytes(), ver.tobytes()))
    assert results[0] == results[1]
    # and through the Python methods, state_of left out
    a, b = new_states(n), new_states(n)
    ra = hasher.update_chunks(a, buf, off, [len(p) for p in piece], final=final)
    rb = hasher.update_chunks_seq(b, buf, off, [len(p) for p in piece], final=final)
    assert np.array_equal(ra, rb) and a.tobytes() == b.tobytes()
    assert [bytes(r) for r in rb[1::2]] == [sha1(p) for p in piece[1::2]]


def test_store_restore_and_continue_through_both_calls(hasher):
    """A chunk fed through update_chunks_seq (three pieces), stored as bytes,
    restored, continued through update_chunks (one piece), and finished through
    update_chunks_seq again (two pieces, the second final)."""
    rng = np.random.default_rng(9)
    n = 6
    parts = [[rnd(rng, rng.integers(0, 400)) for _ in range(6)] for _ in range(n)]
    arena = Arena(9)
    off = [[arena.put(p) for p in row] for row in parts]
    buf = arena.buffer()
    states = new_states(n)
    so = [c for c in range(n) for _ in range(3)]
    out = hasher.update_chunks_seq(states, buf, [off[c][j] for c in range(n) for j in range(3)],
                                   [len(parts[c][j]) for c in range(n) for j in range(3)], state_of=so)
    assert not out.any()
    stored = states.tobytes()
    restored = np.frombuffer(stored, dtype=STATE_DTYPE).copy()
    out = hasher.update_chunks(restored, buf, [off[c][3] for c in range(n)], [len(parts[c][3]) for c in range(n)])
    assert not out.any()
    assert restored["total"].tolist() == [sum(len(p) for p in row[:4]) for row in parts]
    so = [c for c in range(n) for _ in range(2)]
    out = hasher.update_chunks_seq(restored, buf, [off[c][j] for c in range(n) for j in (4, 5)],
                                   [len(parts[c][j]) for c in range(n) for j in (4, 5)], state_of=so,
                                   final=[0, 1] * n)
    assert [bytes(r) for r in out[1::2]] == [sha1(b"".join(row)) for row in parts]
    assert not out[0::2].any()
    assert restored.tobytes() == new_states(n).tobytes()


def test_chains_straddle_launches(monkeypatch):
    """LBF_UPDATE_MB=1: three chains whose pieces (one of them larger than a
    launch, between two small ones) spread over several launches in caller
    order."""
    from bitflood_amd import ChunkHasher
    monkeypatch.setenv("LBF_UPDATE_MB", "1")
    rng = np.random.default_rng(10)
    sizes = [[5, (2 << 20) + 77, 9], [700000, 700001, 3], [1, 0, 600000]]
    parts = [[rnd(rng, s) for s in row] for row in sizes]
    arena = Arena(None)
    order = [(c, j) for j in range(3) for c in range(3)]
    off = [arena.put(parts[c][j]) for c, j in order]
    buf = arena.buffer()
    with ChunkHasher(device_mask=1) as h:
        states = new_states(3)
        out = h.update_chunks_seq(states, buf, off, [len(parts[c][j]) for c, j in order],
                                  state_of=[c for c, _ in order], final=[j == 2 for _, j in order])
    assert [bytes(r) for r in out[6:]] == [sha1(b"".join(row)) for row in parts]
    assert not out[:6].any() and states.tobytes() == new_states(3).tobytes()


def test_batch_refusals_leave_everything_untouched(hasher):
    rng = np.random.default_rng(11)
    buf = rng.integers(0, 256, 1000, dtype=np.uint8)
    states = new_states(4)
    hasher.update_chunks(states, buf, [0, 10, 20, 30], [5, 70, 0, 64])
    corrupt = states.copy()
    corrupt["buffered"][1] = 7  # total is 70: should be 6
    big = states.copy()
    big["total"][2] = 2**61 - 15  # 10 + 10 fit no more, each alone would
    big["buffered"][2] = (2**61 - 15) % 64
    ones = np.ones(3, dtype=np.uint8)
    cases = [
        ("is final", 0, states, [100, 200, 300], [10, 10, 10], [2, 0, 2], ones),
        ("corrupt state", 1, corrupt, [100, 200, 300], [10, 10, 10], [0, 1, 1], None),
        ("outside", 1, states, [100, 995, 300], [10, 6, 10], [0, 0, 2], None),
        ("names state 4", 2, states, [100, 200, 300], [10, 10, 10], [0, 0, 4], None),
        ("2^61", 2, big, [100, 200, 300], [10, 10, 10], [2, 0, 2], None),
    ]
    for what, piece, st, offs, sizes, so, fin in cases:
        st = st.copy()
        before = st.tobytes()
        dig = np.full((3, 20), FILL, dtype=np.uint8)
        ver = np.full(3, FILL, dtype=np.uint8)
        rc = raw_batch(hasher, "lbf_sha1_update_seq_batch", st, buf, offs, sizes, so, fin, dig,
                       np.zeros((3, 20), np.uint8), ver)
        msg = _capi.load().lbf_last_error().decode()
        assert rc == _capi.LBF_ERR_INVALID and what in msg and f"piece {piece} " in msg, (what, rc, msg)
        assert st.tobytes() == before and (dig == FILL).all() and (ver == FILL).all(), what
    # what update_chunks refuses as "the second piece" is accepted here, and the context still works
    with pytest.raises(LbfError):
        hasher.update_chunks(states, buf, [100, 200], [10, 10], state_of=[1, 1])
    got = hasher.update_chunks_seq(states, buf, [100, 200, 0], [10, 10, 0], state_of=[1, 1, 1], final=[0, 0, 1])
    assert bytes(got[2]) == sha1(buf[10:80].tobytes() + buf[100:110].tobytes() + buf[200:210].tobytes())


def test_chain_table_drives_the_launch():
    """hashing.chain_table lays a caller's interleaved pieces out for the
    launch: arrays in arr[order], results back at order[j]."""
    rng = np.random.default_rng(12)
    state_of = np.array([3, 1, 3, 0, 1, 3, 3], dtype=np.uint32)
    data = [rnd(rng, rng.integers(1, 150)) for _ in state_of]
    fin = np.array([0, 0, 0, 1, 1, 0, 1], dtype=np.uint8)
    order, chain_state, chain_first = chain_table(state_of)
    chains = [(int(s), [(data[i], bool(fin[i])) for i in order[chain_first[c]:chain_first[c + 1]]])
              for c, s in enumerate(chain_state)]
    assert [s for s, _ in chains] == [3, 1, 0]
    run_launch(chains, 4, phase=1)


def test_one_piece_and_seq_calls_agree_over_cut_pieces_and_launches(monkeypatch):
    """The calls that take one piece per state and the seq calls, given the same
    pieces with no state repeated, through launches that multiply and a piece
    that is cut: states after each call, digests, verdicts, and for text the
    slots and lengths, are equal between the two and to hashlib.  Five chains of
    0, 1, 63, 64 and 200 bytes, two calls per chain, the second final with
    expected digests of which one is wrong.  A context's launches hold 1 MiB at
    the least (LBF_UPDATE_MB=1), so a sixth chain brings a piece of 1 MiB + 200
    bytes: it is cut, and every call is several launches."""
    from bitflood_amd import ChunkHasher
    from tests import wire_layouts as W
    monkeypatch.setenv("LBF_UPDATE_MB", "1")
    rng = np.random.default_rng(77)
    first = [0, 1, 63, 64, 200, (1 << 20) + 200]
    second = [1, 63, 64, 200, 0, 77]
    state_of = [3, 0, 4, 1, 5, 2]  # no state repeats
    n = len(first)
    calls = [[rnd(rng, s) for s in first], [rnd(rng, s) for s in second]]
    arena = Arena(3)
    offs = [[arena.put(p) for p in call] for call in calls]
    buf = arena.buffer()
    whole = [calls[0][k] + calls[1][k] for k in range(n)]
    expected = np.array([np.frombuffer(sha1(w), dtype=np.uint8) for w in whole])
    expected[2, 7] ^= 0x10  # one digest is wrong
    mid = {state_of[k]: sha1_model.update(sha1_model.init(), calls[0][k]) for k in range(n)}
    with ChunkHasher(device_mask=1) as h:
        results = []
        for fn in ("lbf_sha1_update_batch", "lbf_sha1_update_seq_batch"):
            st = new_states(n)
            dig = np.full((n, 20), FILL, dtype=np.uint8)
            ver = np.full(n, FILL, dtype=np.uint8)
            assert raw_batch(h, fn, st, buf, offs[0], first, state_of, None, None, None, None) == 0
            check_states(st, n, mid, new_states(n))
            after_first = st.tobytes()
            assert raw_batch(h, fn, st, buf, offs[1], second, state_of, [1] * n, dig, expected, ver) == 0
            assert [bytes(d) for d in dig] == [sha1(w) for w in whole], fn
            assert ver.tolist() == [1, 1, 0, 1, 1, 1], fn
            assert st.tobytes() == new_states(n).tobytes()
            results.append((after_first, dig.tobytes(), ver.tobytes()))
        assert results[0] == results[1]

        # text: chunks of 0, 57 and 130 bytes in the encoder's layout, and one whose text is larger than a launch
        chunks = [b"", rnd(rng, 57), rnd(rng, 130), rnd(rng, 800000)]
        texts = [W.xmlrpc_text(c) for c in chunks]
        assert len(texts[3]) > (1 << 20)
        slots = np.concatenate([[5], 5 + np.cumsum([len(c) + 3 for c in chunks])[:-1]]).astype(np.uint64)
        caps = [len(c) for c in chunks]
        exp = np.array([np.frombuffer(sha1(c), dtype=np.uint8) for c in chunks])
        exp[1, 0] ^= 1  # one digest is wrong
        want = np.full(int(slots[-1]) + caps[-1] + 9, FILL, dtype=np.uint8)
        for c, s in zip(chunks, slots):
            want[int(s):int(s) + len(c)] = np.frombuffer(c, dtype=np.uint8)
        for split in (1, 74):
            runs = []
            for fn in (h.update_text, h.update_text_seq):
                b64, sha, out = new_b64_states(4), new_states(4), np.full_like(want, FILL)
                stages = []
                for final, pieces in ((0, [t[:split] for t in texts]), (1, [t[split:] for t in texts])):
                    lens = [len(p) for p in pieces]
                    toff = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
                    sizes, ver = fn(b64, sha, np.frombuffer(b"".join(pieces) + b"\0", dtype=np.uint8), toff, lens, out,
                                    slots, caps, state_of=[2, 0, 3, 1], final=[final] * 4, expected=exp)
                    stages.append((b64.tobytes(), sha.tobytes(), out.tobytes(), sizes.tolist(), ver.tolist()))
                assert stages[0][3] == [0] * 4 and stages[0][4] == [False] * 4
                assert stages[1][3] == caps and stages[1][4] == [True, False, True, True], split
                assert stages[1][2] == want.tobytes(), split
                runs.append(stages)
            assert runs[0] == runs[1], split

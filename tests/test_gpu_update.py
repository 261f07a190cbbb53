"""Chunks hashed piece by piece on the GPU: resumable SHA-1 states
(lbf_sha1_state, lbf_sha1_update_batch / lbf_sha1_update_launch,
ChunkHasher.update_chunks, libBitFlood::PieceHasher).

Expected values come from hashlib, the oracle and, for forged states no real
chain reaches, tests/sha1_model.py (pinned against both in
tests/test_update_cpu.py) -- never from the one-shot GPU path.  Shapes are the
smallest at which the kernel can go wrong: every buffered x size corner around
the 64-byte block and the 56-byte padding edge, every source phase of the
16-byte load path, waves that are ragged and partly idle.
"""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from bitflood_amd import STATE_DTYPE, ChunkHasher, DeviceBuffer, LbfError, _capi, b64_27, new_states
from bitflood_amd import hashing as H
from tests import sha1_model

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIRST = [0, 1, 8, 55, 56, 63, 64]
SECOND = [0, 1, 7, 8, 9, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 200]


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


def digests_of(chunks) -> np.ndarray:
    return np.frombuffer(b"".join(sha1(c) for c in chunks), dtype=np.uint8).reshape(-1, 20)


class Arena:
    """Pieces laid out in one buffer, each at a chosen offset mod 16."""

    def __init__(self, phase=0):
        self.phase, self.parts, self.len = phase, [], 0

    def put(self, data: bytes) -> int:
        pad = (self.phase - self.len) % 16
        self.parts.append(bytes(pad) + bytes(data))
        off = self.len + pad
        self.len = off + len(data)
        return off

    def buffer(self) -> np.ndarray:
        return np.frombuffer(b"".join(self.parts) + b"\0", dtype=np.uint8).copy()


@pytest.mark.parametrize("phase", [0, 1, 4, 15])
@pytest.mark.parametrize("final_with_second", [False, True])
def test_every_buffered_size_corner(hasher, phase, final_with_second):
    """One state per (first piece, second piece) size: the second update meets
    `first % 64` buffered bytes and tops the block up with less than, exactly,
    or more than it needs; the final piece pads into one block or two.  The
    final flag comes with the second piece, or alone on a third, empty one."""
    rng = np.random.default_rng(1000 + phase)
    combos = [(a, b) for a in FIRST for b in SECOND]
    n = len(combos)
    arena = Arena(phase)
    data = [(rng.integers(0, 256, a, dtype=np.uint8).tobytes(), rng.integers(0, 256, b, dtype=np.uint8).tobytes())
            for a, b in combos]
    off1 = [arena.put(d[0]) for d in data]
    off2 = [arena.put(d[1]) for d in data]
    buf = arena.buffer()
    assert all(o % 16 == phase for o in off1 + off2)
    states = new_states(n)
    fresh = new_states(n).tobytes()
    out = hasher.update_chunks(states, buf, off1, [a for a, _ in combos])
    assert not out.any()
    assert states["total"].tolist() == [a for a, _ in combos]
    assert states["buffered"].tolist() == [a % 64 for a, _ in combos]
    flags = np.ones(n, dtype=bool)
    if final_with_second:
        got = hasher.update_chunks(states, buf, off2, [b for _, b in combos], final=flags)
    else:
        out = hasher.update_chunks(states, buf, off2, [b for _, b in combos])
        assert not out.any()
        assert states["total"].tolist() == [a + b for a, b in combos]
        assert states["buffered"].tolist() == [(a + b) % 64 for a, b in combos]
        for k, (a, b) in enumerate(combos):  # the kept bytes are the chunk's last ones
            r = (a + b) % 64
            assert states["block"][k][:r].tobytes() == (data[k][0] + data[k][1])[a + b - r:], (a, b)
        got = hasher.update_chunks(states, buf, np.zeros(n, dtype=np.uint64), np.zeros(n, dtype=np.uint32),
                                   final=flags)
    want = digests_of(d[0] + d[1] for d in data)
    bad = [combos[k] for k in range(n) if not np.array_equal(got[k], want[k])]
    assert not bad, bad
    assert states.tobytes() == fresh  # Final() restarts every state


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_waves(hasher, oracle, n):
    """Chunks of 0..5,000 bytes, different in every lane, each fed in three to
    eight calls at random cut points; chains that have ended sit out the later
    calls, so the waves go ragged."""
    rng = np.random.default_rng(7000 + n)
    sizes = rng.integers(0, 5001, n)
    chunks = [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in sizes]
    arena = Arena(phase=3)
    start = [arena.put(c) for c in chunks]
    buf = arena.buffer()
    calls = rng.integers(3, 9, n)
    cuts = [[0] + sorted(rng.integers(0, int(sizes[c]) + 1, int(calls[c]) - 1).tolist()) + [int(sizes[c])]
            for c in range(n)]
    states = new_states(n)
    got = np.zeros((n, 20), dtype=np.uint8)
    for r in range(8):
        live = [c for c in range(n) if calls[c] > r]
        offs = [start[c] + cuts[c][r] for c in live]
        szs = [cuts[c][r + 1] - cuts[c][r] for c in live]
        fin = [calls[c] == r + 1 for c in live]
        out = hasher.update_chunks(states, buf, offs, szs, state_of=live, final=fin)
        for k, c in enumerate(live):
            if fin[k]:
                got[c] = out[k]
            else:
                assert not out[k].any()
    assert np.array_equal(got, digests_of(chunks))
    assert [b64_27(bytes(d)) for d in got] == [oracle.base64_encode(np.frombuffer(c, dtype=np.uint8)) for c in chunks]
    assert states.tobytes() == new_states(n).tobytes()


def _raw_update(hasher, states, buf, offs, sizes, state_of, final, digests, expected, verdicts):
    """lbf_sha1_update_batch with the caller's own output arrays."""
    offs = np.ascontiguousarray(offs, dtype=np.uint64)
    sizes = np.ascontiguousarray(sizes, dtype=np.uint32)
    so = None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32)
    fin = None if final is None else np.ascontiguousarray(final, dtype=np.uint8)
    p = lambda a: None if a is None else a.ctypes.data  # noqa: E731
    return _capi.load().lbf_sha1_update_batch(hasher._h, states.ctypes.data, states.size, p(so), buf.ctypes.data,
                                              buf.size, offs.ctypes.data, sizes.ctypes.data, p(fin), offs.size,
                                              p(digests), p(expected), p(verdicts))


def test_state_of_touches_only_its_states_and_final_entries(hasher):
    """40 pieces on a shuffled subset of 300 states, half of them final:
    the other states stay byte-identical, digest and verdict entries of the
    pieces that are not final keep their 0xEE, and a final piece leaves its
    state as new_states gives it."""
    rng = np.random.default_rng(300)
    n_states, n = 300, 40
    states = new_states(n_states)
    # every state mid-chunk already, each with its own bytes
    pre = [rng.integers(0, 256, int(rng.integers(1, 200)), dtype=np.uint8).tobytes() for _ in range(n_states)]
    arena = Arena(phase=5)
    pre_off = [arena.put(p) for p in pre]
    subset = rng.permutation(n_states)[:n]
    piece = [rng.integers(0, 256, int(rng.integers(0, 700)), dtype=np.uint8).tobytes() for _ in range(n)]
    off = [arena.put(p) for p in piece]
    buf = arena.buffer()
    hasher.update_chunks(states, buf, pre_off, [len(p) for p in pre])
    before = states.copy()
    final = (np.arange(n) % 2).astype(np.uint8)
    want = digests_of(pre[s] + piece[k] for k, s in enumerate(subset))
    expected = want.copy()
    expected[::3, 7] ^= 0x10  # every third expected digest is wrong
    dig = np.full((n, 20), 0xEE, dtype=np.uint8)
    ver = np.full(n, 0xEE, dtype=np.uint8)
    assert _raw_update(hasher, states, buf, off, [len(p) for p in piece], subset, final, dig, expected, ver) == 0
    for k, s in enumerate(subset):
        if final[k]:
            assert np.array_equal(dig[k], want[k]), k
            assert ver[k] == (0 if k % 3 == 0 else 1), k
            assert states[s].tobytes() == new_states(1).tobytes()
        else:
            assert (dig[k] == 0xEE).all() and ver[k] == 0xEE, k
            assert states["total"][s] == len(pre[s]) + len(piece[k])
    untouched = np.setdiff1d(np.arange(n_states), subset)
    assert states[untouched].tobytes() == before[untouched].tobytes()
    # the chains that went on finish right
    rest = [k for k in range(n) if not final[k]]
    got = hasher.update_chunks(states, buf, np.zeros(len(rest)), np.zeros(len(rest)), state_of=subset[rest],
                               final=np.ones(len(rest)))
    assert np.array_equal(got, want[rest])


def test_verify_verdicts(hasher):
    rng = np.random.default_rng(33)
    n = 100
    chunks = [rng.integers(0, 256, int(rng.integers(0, 3000)), dtype=np.uint8).tobytes() for _ in range(n)]
    arena = Arena()
    start = [arena.put(c) for c in chunks]
    buf = arena.buffer()
    half = [len(c) // 2 for c in chunks]
    states = new_states(n)
    expected = digests_of(chunks).copy()
    expected[::3, 19] ^= 1
    ver = hasher.update_chunks(states, buf, start, half, expected=expected)
    assert ver.dtype == bool and not ver.any()  # nothing is final yet
    ver = hasher.update_chunks(states, buf, [s + h for s, h in zip(start, half)],
                               [len(c) - h for c, h in zip(chunks, half)], final=np.ones(n), expected=expected)
    assert ver.tolist() == [k % 3 != 0 for k in range(n)]


def test_forged_states_keep_the_length_in_64_bits(hasher):
    """States as a chain would be after 2^29 - 64, 2^32 - 64 and 2^32 + 2^29 -
    125 bytes: 200 more bytes and the final padding take the bit count through
    2^32 and the byte count through 2^32.  Checked against the Python model
    continued from the same forged state."""
    rng = np.random.default_rng(64)
    totals = [2**29 - 64, 2**32 - 64, 2**32 + 2**29 - 128 + 3, 2**29 - 64 + 61]
    n = len(totals)
    states = new_states(n)
    tail = rng.integers(0, 256, (n, 200), dtype=np.uint8)
    want = []
    for k, t in enumerate(totals):
        h = rng.integers(0, 2**32, 5, dtype=np.uint64).astype(np.uint32)
        blk = rng.integers(0, 256, 64, dtype=np.uint8)
        states["h"][k], states["total"][k], states["buffered"][k], states["block"][k] = h, t, t % 64, blk
        st = ([int(x) for x in h], t, blk[:t % 64].tobytes())
        want.append(sha1_model.final(sha1_model.update(st, tail[k].tobytes())))
    got = hasher.update_chunks(states, tail.reshape(-1), np.arange(n) * 200, np.full(n, 200), final=np.ones(n))
    assert [bytes(g) for g in got] == want
    assert states.tobytes() == new_states(n).tobytes()


def test_suspend_and_resume_in_a_new_context():
    rng = np.random.default_rng(9)
    n = 70
    chunks = [rng.integers(0, 256, int(rng.integers(0, 4000)), dtype=np.uint8).tobytes() for _ in range(n)]
    arena = Arena(phase=9)
    start = [arena.put(c) for c in chunks]
    buf = arena.buffer()
    cut = [int(rng.integers(0, len(c) + 1)) for c in chunks]
    with ChunkHasher(device_mask=1) as h1:
        states = new_states(n)
        h1.update_chunks(states, buf, start, cut)
        stored = states.tobytes()
    del states
    assert len(stored) == 96 * n
    with ChunkHasher(device_mask=1) as h2:
        resumed = np.frombuffer(stored, dtype=STATE_DTYPE).copy()
        got = h2.update_chunks(resumed, buf, [s + c for s, c in zip(start, cut)],
                               [len(c) - k for c, k in zip(chunks, cut)], final=np.ones(n))
    assert np.array_equal(got, digests_of(chunks))


@pytest.mark.parametrize("registered", [False, True])
def test_call_larger_than_a_launch_is_split(monkeypatch, registered):
    """LBF_UPDATE_MB=1: pieces of 3 MiB + 65, 1 MiB and 5 bytes in one call run
    as several launches, the first piece cut at multiples of 64 bytes."""
    monkeypatch.setenv("LBF_UPDATE_MB", "1")
    rng = np.random.default_rng(77)
    sizes = [(3 << 20) + 65, 1 << 20, 5]
    # page-aligned, whole pages: a registered range shares no page with anything else
    total = sum(sizes) + 2 * 7
    raw = np.zeros(total + 2 * 4096, dtype=np.uint8)
    lead = (-raw.ctypes.data) % 4096
    buf = raw[lead:lead + (total + 4095) // 4096 * 4096]
    buf[:] = rng.integers(0, 256, buf.size, dtype=np.uint8)
    offs = [3, 3 + sizes[0] + 7, 3 + sizes[0] + 7 + sizes[1] + 4]
    with ChunkHasher(device_mask=1) as h:
        if registered:
            h.register_host(buf)
        states = new_states(3)
        # the chains are mid-block already, so the cuts do not fall on block edges of the chain
        h.update_chunks(states, buf, [0, 0, 0], [3, 0, 1])
        got = h.update_chunks(states, buf, offs, sizes, final=[1, 1, 1])
        if registered:
            h.unregister_host(buf)
    want = digests_of([buf[:3].tobytes() + buf[offs[0]:offs[0] + sizes[0]].tobytes(),
                       buf[offs[1]:offs[1] + sizes[1]].tobytes(),
                       buf[:1].tobytes() + buf[offs[2]:offs[2] + sizes[2]].tobytes()])
    assert np.array_equal(got, want)
    assert states.tobytes() == new_states(3).tobytes()


def test_device_resident_launch_on_a_caller_stream():
    """update_launch with everything in DeviceBuffers: two launches per chain
    on one stream; a piece whose state index is n_states is skipped and its
    neighbours stay exact; a digest array sized for fewer pieces is refused."""
    lib = _capi.load()
    rng = np.random.default_rng(5)
    n, n_states = 9, 12
    chunks = [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in [0, 1, 63, 64, 65, 1000, 4097, 130, 56]]
    arena = Arena(phase=2)
    start = [arena.put(c) for c in chunks]
    buf = arena.buffer()
    cut = [len(c) // 3 for c in chunks]
    state_of = np.array([11, 3, 0, n_states, 7, 1, 10, 2, 5], dtype=np.uint32)  # piece 3 names no state
    stream = ctypes.c_void_p()
    _capi.check(lib.lbf_stream_create(ctypes.byref(stream)))
    bufs = {k: DeviceBuffer(b) for k, b in dict(states=96 * n_states, so=4 * n, data=buf.size, off=8 * n, size=4 * n,
                                                fin=n, dig=20 * n, exp=20 * n, ver=n, small=20 * (n - 1)).items()}
    try:
        bufs["states"].upload(new_states(n_states))
        bufs["so"].upload(state_of)
        bufs["data"].upload(buf)
        bufs["dig"].upload(np.full(20 * n, 0xEE, dtype=np.uint8))
        bufs["ver"].upload(np.full(n, 0xEE, dtype=np.uint8))
        want = digests_of(chunks)
        expected = want.copy()
        expected[4, 0] ^= 0x80
        bufs["exp"].upload(expected)
        # first pieces: no final flags, no outputs
        bufs["off"].upload(np.array(start, dtype=np.uint64))
        bufs["size"].upload(np.array(cut, dtype=np.uint32))
        H.update_launch(bufs["states"], n_states, bufs["so"], bufs["data"], bufs["off"], bufs["size"], None, n, None,
                        stream=stream)
        _capi.check(lib.lbf_stream_synchronize(stream))  # the tables are reused below
        mid = bufs["states"].download(96 * n_states).view(STATE_DTYPE)
        for k in range(n):
            if k != 3:
                assert mid["total"][state_of[k]] == cut[k]
        assert mid[[4, 6, 8, 9]].tobytes() == new_states(4).tobytes()  # states no piece names
        # a digest array sized for fewer pieces is refused before anything runs
        bufs["off"].upload(np.array([s + c for s, c in zip(start, cut)], dtype=np.uint64))
        bufs["size"].upload(np.array([len(c) - k for c, k in zip(chunks, cut)], dtype=np.uint32))
        bufs["fin"].upload(np.ones(n, dtype=np.uint8))
        with pytest.raises(LbfError) as e:
            H.update_launch(bufs["states"], n_states, bufs["so"], bufs["data"], bufs["off"], bufs["size"], bufs["fin"],
                            n, bufs["small"], stream=stream)
        assert e.value.status == _capi.LBF_ERR_INVALID and "digests" in str(e.value), str(e.value)
        with pytest.raises(LbfError) as e:
            H.update_launch(bufs["states"], n_states + 1, bufs["so"], bufs["data"], bufs["off"], bufs["size"],
                            bufs["fin"], n, bufs["dig"], stream=stream)
        assert e.value.status == _capi.LBF_ERR_INVALID and "states" in str(e.value), str(e.value)
        with pytest.raises(LbfError) as e:
            H.update_launch(bufs["states"].ptr + 8, n_states - 1, bufs["so"], bufs["data"], bufs["off"], bufs["size"],
                            bufs["fin"], n, bufs["dig"], stream=stream)
        assert e.value.status == _capi.LBF_ERR_INVALID and "16-byte" in str(e.value), str(e.value)
        H.update_launch(bufs["states"], n_states, bufs["so"], bufs["data"], bufs["off"], bufs["size"], bufs["fin"], n,
                        bufs["dig"], bufs["exp"], bufs["ver"], stream=stream)
        _capi.check(lib.lbf_stream_synchronize(stream))
        dig = bufs["dig"].download(20 * n).reshape(n, 20)
        ver = bufs["ver"].download(n)
        for k in range(n):
            if k == 3:
                assert (dig[k] == 0xEE).all() and ver[k] == 0xEE
            else:
                assert np.array_equal(dig[k], want[k]), k
                assert ver[k] == (0 if k == 4 else 1)
        assert bufs["states"].download(96 * n_states).tobytes() == new_states(n_states).tobytes()
    finally:
        for b in bufs.values():
            b.free()
        _capi.check(lib.lbf_stream_destroy(stream))


def test_host_path_refusals_leave_states_and_outputs_untouched(hasher):
    rng = np.random.default_rng(2)
    buf = rng.integers(0, 256, 1000, dtype=np.uint8)
    states = new_states(4)
    hasher.update_chunks(states, buf, [0, 10, 20, 30], [5, 70, 0, 64])
    corrupt = states.copy()
    corrupt["buffered"][1] = 7  # total is 70: should be 6
    over = states.copy()
    over["buffered"][1] = 70
    cases = [
        ("second piece", states, [100, 200, 300], [10, 10, 10], [2, 0, 2]),
        ("corrupt state", corrupt, [100, 200, 300], [10, 10, 10], [0, 1, 2]),
        ("corrupt state", over, [100, 200, 300], [10, 10, 10], [0, 1, 2]),
        ("outside", states, [100, 995, 300], [10, 6, 10], [0, 1, 2]),
        ("names state 4", states, [100, 200, 300], [10, 10, 10], [0, 4, 2]),
    ]
    for what, st, offs, sizes, so in cases:
        st = st.copy()
        before = st.tobytes()
        dig = np.full((3, 20), 0xEE, dtype=np.uint8)
        ver = np.full(3, 0xEE, dtype=np.uint8)
        rc = _raw_update(hasher, st, buf, offs, sizes, so, np.ones(3, dtype=np.uint8), dig, np.zeros((3, 20), np.uint8),
                         ver)
        msg = _capi.load().lbf_last_error().decode()
        assert rc == _capi.LBF_ERR_INVALID and what in msg and "piece " in msg, (what, rc, msg)
        assert st.tobytes() == before and (dig == 0xEE).all() and (ver == 0xEE).all(), what
    with pytest.raises(LbfError):
        hasher.update_chunks(states, buf, [100, 200], [10, 10], state_of=[1, 1])
    # and the context still works
    got = hasher.update_chunks(states, buf, [100, 200, 300, 400], [0, 0, 0, 0], final=np.ones(4))
    assert np.array_equal(got, digests_of([buf[0:5], buf[10:80], b"", buf[30:94]]))


def test_cpp_piece_hasher():
    out = subprocess.run([os.path.join(ROOT, "bitflood_amd", "lib", "lbf_piece_tests")], capture_output=True, text=True,
                         timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "piece_tests OK" in out.stdout

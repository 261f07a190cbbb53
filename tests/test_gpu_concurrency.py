"""Concurrent callers on one lbf_ctx, and several contexts at once.

The reference's Base64Encode builds its hasher on the stack per call, so any
number of threads may call it (/root/reference/cpp/src/Encoder.cpp:107-120;
SURVEY.md §8b).  The drop-in keeps that promise with one context per process
whose calls serialize on the context (staging.cpp run_job / run_device_job)
and a thread-local last-error string.  These tests hammer one context from
several host threads (ctypes drops the GIL for the call, so the calls really
overlap on the host) with a mix of hash, verify, one-buffer and file batches,
including failing calls, and check every result against hashlib bit for bit.

The piecewise calls (update_text, update_chunks) and the wire calls (verify_b64,
verify_encode_b64) share worker 0's first stream, the context's mutex, its
counters and, the two update calls, one scratch allocation grown on demand;
the three decode switches are process-wide and read at enqueue time.  The
second half of this file runs them from eight threads at once, with a ninth
flipping the switches, against the Python models of tests/wire_layouts.py,
tests/wire_piece_model.py and tests/sha1_model.py, Feed (tests/
test_gpu_b64_update.py) checking every call whole.
"""
import functools
import hashlib
import os
import threading

import numpy as np
import pytest

from bitflood_amd import ChunkHasher, LbfError, chunk_table, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import stream_feed as S
from tests import wire_flat_model as F
from tests import wire_layouts as W
from tests import wire_piece_model as M
from tests.test_gpu_b64_update import Feed, _ragged_chains
from tests.test_gpu_update import Arena, digests_of

pytestmark = pytest.mark.gpu


def _table(rng, buf_len, n):
    sizes = rng.integers(0, 200000, n).astype(np.uint32)
    offs = np.array([rng.integers(0, buf_len - s + 1) for s in sizes], dtype=np.uint64)
    return offs, sizes


def _want(buf, offs, sizes):
    return np.frombuffer(b"".join(hashlib.sha1(buf[o:o + s].tobytes()).digest() for o, s in zip(offs, sizes)),
                         dtype=np.uint8).reshape(-1, 20)


def _run_threads(target, n):
    errors = []

    def wrap(t):
        try:
            target(t)
        except BaseException as e:  # collected, re-raised in the main thread
            errors.append((t, e))

    th = [threading.Thread(target=wrap, args=(t,), daemon=True) for t in range(n)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=300)
    assert not any(x.is_alive() for x in th), "a caller thread did not finish"
    assert not errors, errors[:3]


@pytest.mark.parametrize("workers", [1, 2])
def test_many_threads_one_context(tmp_path, monkeypatch, workers):
    monkeypatch.setenv("LBF_WORKERS_PER_DEVICE", str(workers))
    rng = np.random.default_rng(404 + workers)
    buf = rng.integers(0, 256, 24 << 20, dtype=np.uint8)
    path = tmp_path / "shared.bin"
    buf[: 8 << 20].tofile(path)
    file_offs, file_sizes = chunk_table(8 << 20, 65536)
    file_want = _want(buf, file_offs, file_sizes)
    with ChunkHasher() as h:
        assert h.num_workers == workers

        def caller(t):
            r = np.random.default_rng(1000 * workers + t)
            for it in range(6):
                kind = (t + it) % 4
                if kind == 0:  # hash batch, ragged and unaligned
                    offs, sizes = _table(r, buf.size, int(r.integers(1, 400)))
                    got = h.hash_chunks(buf, offs, sizes)
                    assert np.array_equal(got, _want(buf, offs, sizes)), (t, it)
                elif kind == 1:  # verify batch with some corrupted expectations
                    offs, sizes = _table(r, buf.size, int(r.integers(1, 300)))
                    exp = _want(buf, offs, sizes).copy()
                    bad = r.random(exp.shape[0]) < 0.3
                    exp[bad, int(r.integers(0, 20))] ^= 0x40
                    assert np.array_equal(h.verify_chunks(buf, offs, sizes, exp), ~bad), (t, it)
                elif kind == 2:  # Base64Encode-style single buffers
                    for _ in range(5):
                        o = int(r.integers(0, buf.size - 70000))
                        n = int(r.integers(0, 70000))
                        assert h.sha1(buf[o:o + n]) == hashlib.sha1(buf[o:o + n].tobytes()).digest(), (t, it)
                else:  # file batch, and a failing call whose message stays in this thread
                    assert np.array_equal(h.hash_file(str(path), file_offs, file_sizes), file_want), (t, it)
                    with pytest.raises(LbfError, match="outside"):
                        h.hash_chunks(buf[:1000], np.array([999], np.uint64), np.array([2], np.uint32))

        _run_threads(caller, 8)


def test_contexts_in_parallel():
    """Several contexts (each with its own staging and streams) used at once."""
    rng = np.random.default_rng(77)
    buf = rng.integers(0, 256, 16 << 20, dtype=np.uint8)
    offs, sizes = chunk_table(buf.size, 262144)
    want = _want(buf, offs, sizes)
    ctxs = [ChunkHasher() for _ in range(3)]
    try:
        def caller(t):
            for _ in range(4):
                assert np.array_equal(ctxs[t % 3].hash_chunks(buf, offs, sizes), want), t
                assert ctxs[t % 3].verify_chunks(buf, offs, sizes, want).all(), t

        _run_threads(caller, 6)
    finally:
        for c in ctxs:
            c.close()


# ------------------------------------------------------------ the piecewise and wire calls
@functools.lru_cache(maxsize=None)
def _text_chains(v):
    """40 chains in mixed layouts: stream v's ragged encoder-layout and unbroken
    chains, one big one per layout (the third changes layout twice), the
    cap + 1 and cap - 1 pair, and eleven more ragged ones."""
    chains = S.decode_chains(v)[0]
    chains = list(chains[:27]) + list(chains[30:32]) + _ragged_chains(11, 8300 + v)
    assert len(chains) == 40 and not all(c.verdict for c in chains)
    return tuple(chains)


def _run_text_feed(h, v, t):
    """The chains through update_text, every call checked whole; returns the characters passed."""
    chains = _text_chains(v)
    Feed(chains, sphase=(None if t % 2 else t % 16), tphase=(None if t % 3 else 5)).run(h)
    return sum(len(p) for c in chains for p in c.pieces)


@functools.lru_cache(maxsize=None)
def _update_work(v):
    """50 chunks of 0..5,000 bytes in three cuts; the records after the first and
    the second call are sha1_model's (through M.sha_state, which keeps the
    chaining values)."""
    rng = np.random.default_rng(6100 + v)
    chunks = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 5001, 50)]
    arena = Arena(phase=(5 * v + 1) % 16)
    start = [arena.put(c) for c in chunks]
    buf = arena.buffer()
    buf.flags.writeable = False
    cuts = [[0] + sorted(rng.integers(0, len(c) + 1, 2).tolist()) + [len(c)] for c in chunks]
    mid = [M.sha_records([M.sha_state(c[:k[r + 1]], len(c)) for c, k in zip(chunks, cuts)], H.STATE_DTYPE)
           for r in range(2)]
    return chunks, start, buf, cuts, mid, digests_of(chunks)


def _run_update_feed(h, v):
    chunks, start, buf, cuts, mid, want = _update_work(v)
    n = len(chunks)
    states = new_states(n)
    for r in range(3):
        got = h.update_chunks(states, buf, [s + k[r] for s, k in zip(start, cuts)], [k[r + 1] - k[r] for k in cuts],
                              final=(np.ones(n) if r == 2 else None))
        if r < 2:
            assert not got.any(), r
            bad = M.sha_records_differ(states, mid[r])
            assert not bad, (r, bad[:3], states[bad[0]], mid[r][bad[0]])
    assert np.array_equal(got, want)
    assert states.tobytes() == new_states(n).tobytes()


@functools.lru_cache(maxsize=None)
def _wire_work(v):
    """30 texts in the encoder's layout and unbroken, every third damaged, with
    W.decode's answer for each; and 30 chunks with the encoder's text, every
    4th expected digest wrong."""
    rng = np.random.default_rng(6200 + v)
    datas = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(1, 5001, 30)]
    texts = [(W.xmlrpc_text if i % 2 == 0 else F.text)(d) for i, d in enumerate(datas)]
    for i in range(0, 30, 3):
        kind = W.KINDS[(i // 3 + v) % len(W.KINDS)]
        places = W.positions(len(texts[i]), kind)
        texts[i] = W.damage(texts[i], kind, places[int(rng.integers(0, len(places)))])
    parts, toff, pos = [], [], 0
    for i, t in enumerate(texts):
        gap = (b"A=" * 8)[:(i + v) % 5]  # characters a decode must not read as the chunk's
        parts += [gap, t]
        toff.append(pos + len(gap))
        pos += len(gap) + len(t)
    text = np.frombuffer(b"".join(parts) + b"A=", dtype=np.uint8)
    caps = np.array([len(d) for d in datas], dtype=np.uint32)
    ooff, pos = [], 7
    for i, d in enumerate(datas):
        pos += 7 * i % 21
        ooff.append(pos)
        pos += len(d)
    want_out = np.full(pos + 13, 0x5A, dtype=np.uint8)
    sizes, verdicts = [], []
    for i, (t, d) in enumerate(zip(texts, datas)):
        w = W.decode(t)
        want_out[ooff[i]:ooff[i] + len(d)] = np.frombuffer(w[:len(d)].ljust(len(d), b"\0"), dtype=np.uint8)
        sizes.append(len(w) if len(w) <= len(d) else len(d) + 1)
        verdicts.append(w == d)
    assert 20 <= sum(verdicts) < 30
    exp = digests_of(datas)
    # the sender's side
    arena = Arena(phase=(3 * v + 2) % 16)
    start = [arena.put(d) for d in datas]
    wrong = exp.copy()
    wrong[::4, 3] ^= 0x20
    for a in (text, want_out, exp, wrong):
        a.flags.writeable = False
    return dict(text=text, toff=toff, tlen=[len(t) for t in texts], caps=caps, exp=exp, ooff=ooff, want_out=want_out,
                sizes=sizes, verdicts=verdicts, data=arena.buffer(), start=start, wrong=wrong,
                encoded=[W.xmlrpc_text(d) for d in datas])


def _run_wire(h, v):
    """verify_b64, then verify_encode_b64; returns the chunks passed to verify_b64."""
    w = _wire_work(v)
    out = np.full(w["want_out"].size, 0x5A, dtype=np.uint8)
    ver, dec = h.verify_b64(w["text"], w["toff"], w["tlen"], w["caps"], w["exp"], out, w["ooff"])
    bad = np.flatnonzero(out != w["want_out"])
    assert bad.size == 0, (v, bad[:5].tolist())
    assert dec.tolist() == w["sizes"] and ver.tolist() == w["verdicts"], v
    ver, texts = h.verify_encode_b64(w["data"], w["start"], w["caps"], w["wrong"])
    assert ver.tolist() == [i % 4 != 0 for i in range(30)], v
    assert texts == w["encoded"], v
    return 30


def _refused_calls(h, t):
    """One refused call of each family.  The piece each names differs from thread
    to thread, so a message that came from another thread's call would show;
    states and outputs stay as they were."""
    k = 1 + t % 7
    n = k + 1
    # update_text: piece k continues the state piece 0 continues
    b64, sha = new_b64_states(n), new_states(n)
    out = np.full(64 * n, 0xEE, dtype=np.uint8)
    text = np.frombuffer(b"QUJD" * n, dtype=np.uint8)
    so = list(range(n))
    so[k] = 0
    with pytest.raises(LbfError) as e:
        h.update_text(b64, sha, text, 4 * np.arange(n), [4] * n, out, 64 * np.arange(n), [3] * n, state_of=so)
    assert "lbf_b64_update_batch" in str(e.value) and f"piece {k} " in str(e.value) and "second piece" in str(e.value)
    assert b64.tobytes() == new_b64_states(n).tobytes() and sha.tobytes() == new_states(n).tobytes()
    assert (out == 0xEE).all()
    # update_chunks: piece k lies outside the buffer
    buf = np.arange(256, dtype=np.uint8)
    states = new_states(n)
    offs = [10 * i for i in range(n)]
    offs[k] = 250
    with pytest.raises(LbfError) as e:
        h.update_chunks(states, buf, offs, [7] * n, final=np.ones(n))
    assert "lbf_sha1_update_batch" in str(e.value) and f"piece {k} " in str(e.value) and "outside" in str(e.value)
    assert states.tobytes() == new_states(n).tobytes()
    # verify_b64: text range k lies outside the buffer
    toff = [4 * i for i in range(n)]
    toff[k] = text.size - 3
    with pytest.raises(LbfError) as e:
        h.verify_b64(text, toff, [4] * n, [3] * n, np.zeros((n, 20), np.uint8), out, 64 * np.arange(n))
    assert "lbf_b64_verify_batch" in str(e.value) and f"text range {k} outside" in str(e.value)
    assert (out == 0xEE).all()


@pytest.mark.parametrize("flipper", [False, True], ids=["steady", "switches-flipped"])
@pytest.mark.parametrize("workers", [1, 2])
def test_piecewise_and_wire_callers_one_context(monkeypatch, workers, flipper):
    """Eight threads on one context, four iterations each, cycling through a Feed
    of 40 chains, an update_chunks feed, verify_b64 + verify_encode_b64, and
    hash_chunks / verify_chunks with one refused call of each piecewise and wire
    family.  With `flipper` a ninth thread sets the three decode switches in a
    seeded order all the while: every result stays the same.  The context's
    counters add up to what the threads passed."""
    monkeypatch.setenv("LBF_WORKERS_PER_DEVICE", str(workers))
    rng = np.random.default_rng(505 + workers)
    buf = rng.integers(0, 256, 4 << 20, dtype=np.uint8)
    for v in range(4):  # the shared, read-only work and its expected values, before any thread starts
        _text_chains(v), _update_work(v), _wire_work(v)
    chars, chunks = [0] * 8, [0] * 8
    stop = threading.Event()
    before = H.set_b64_fused(True), H.set_b64_lines(True), H.set_b64_flat(True)
    S.set_route(before)
    flips = []

    def flip():
        r = np.random.default_rng(17)
        order = r.integers(0, 3, 4096)
        on = r.integers(0, 2, 4096)
        try:
            while not stop.is_set():
                k = len(flips) % 4096
                (H.set_b64_fused, H.set_b64_lines, H.set_b64_flat)[order[k]](bool(on[k]))
                flips.append(k)
                stop.wait(0.0005)
        finally:
            S.set_route(before)

    with ChunkHasher() as h:
        assert h.num_workers == workers
        u0, f0, w0 = h.b64_update_stats(), h.b64_flat_stats(), h.b64_stats()

        def caller(t):
            r = np.random.default_rng(2000 * workers + t)
            for it in range(4):
                kind, v = (t + it) % 4, (t + 2 * it) % 4
                if kind == 0:
                    chars[t] += _run_text_feed(h, v, t)
                elif kind == 1:
                    _run_update_feed(h, v)
                elif kind == 2:
                    chunks[t] += _run_wire(h, v)
                else:
                    offs, sizes = _table(r, buf.size, int(r.integers(1, 200)))
                    want = _want(buf, offs, sizes)
                    if it % 2:
                        assert np.array_equal(h.hash_chunks(buf, offs, sizes), want), (t, it)
                    else:
                        exp = want.copy()
                        bad = r.random(exp.shape[0]) < 0.3
                        exp[bad, int(r.integers(0, 20))] ^= 0x40
                        assert np.array_equal(h.verify_chunks(buf, offs, sizes, exp), ~bad), (t, it)
                    _refused_calls(h, t)

        fl = threading.Thread(target=flip, daemon=True)
        if flipper:
            fl.start()
        try:
            _run_threads(caller, 8)
        finally:
            stop.set()
            if flipper:
                fl.join(timeout=60)
        assert not fl.is_alive(), "the switch thread did not finish"
        assert not flipper or len(flips) > 8
        u1, f1, w1 = h.b64_update_stats(), h.b64_flat_stats(), h.b64_stats()
    assert (H.set_b64_fused(before[0]), H.set_b64_lines(before[1]), H.set_b64_flat(before[2])) == before
    assert sum(chars) > 0 and sum(chunks) == 8 * 30
    line, scan = u1["line_chars"] - u0["line_chars"], u1["scan_chars"] - u0["scan_chars"]
    assert line + scan == sum(chars), (line, scan, sum(chars))
    assert 0 <= f1["flat_chars"] - f0["flat_chars"] <= scan
    assert w1["one_pass"] - w0["one_pass"] + w1["general"] - w0["general"] == sum(chunks)


def test_piecewise_contexts_in_parallel():
    """Three contexts, two threads each: a Feed and an update_chunks feed per
    thread over shared, read-only source buffers."""
    for v in range(4):
        _text_chains(v), _update_work(v)
    ctxs = [ChunkHasher() for _ in range(3)]
    try:
        def caller(t):
            for it in range(2):
                _run_text_feed(ctxs[t % 3], (t + it) % 4, t)
                _run_update_feed(ctxs[t % 3], (t + 2 * it + 1) % 4)

        _run_threads(caller, 6)
    finally:
        for c in ctxs:
            c.close()

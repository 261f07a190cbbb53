"""lbf_wire_frames_launch and lbf_wire_send_chunks_launch on the GPU against
tests/wire_frame_model.py (which tests/test_wire_frames_cpu.py pins against the
C++): every output array is prefilled and compared whole.  The shapes are the
smallest at which the kernels can go wrong: every start phase of the 16-byte
grid, the edges of a split block, of a search trip and of a compaction group,
one stream and one frame table past one trip of the scan."""
import os
import subprocess

import numpy as np
import pytest

import bitflood_amd as B
from bitflood_amd import hashing as H
from tests import wire_frame_model as M
from tests.test_wire_frames_cpu import build_program

pytestmark = pytest.mark.gpu
FD = H.WIRE_FRAME_DTYPE
EE32, EE64 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
TRIP, BLOCK, GROUP, SCAN = H.WIRE_SEARCH_TRIP, H.WIRE_SPLIT_BLOCK, H.WIRE_BIND_BLOCK, H.WIRE_SCAN_WIDTH


def up(arr):
    arr = np.ascontiguousarray(arr)
    buf = B.DeviceBuffer(max(arr.nbytes, 16))
    if arr.nbytes:
        buf.upload(arr.view(np.uint8).reshape(-1))
    return buf


def filled(n, dtype, value=0xEE):
    return np.frombuffer(bytes([value]) * (n * np.dtype(dtype).itemsize), dtype).copy()


# ---- the split -------------------------------------------------------------
def run_splits(cases):
    """cases = [(stream, phase, max_frames)]: every stream lies at its phase of the 16-byte grid with a '\\n' directly
    before and behind it; all launches first, then one download, each output compared whole."""
    arena, at = bytearray(), []
    for s, phase, _ in cases:
        arena += b"\n" * (-len(arena) % 16 + 16 + phase)
        at.append(len(arena))
        arena += s + b"\n"
    d_arena = up(np.frombuffer(bytes(arena), np.uint8))
    slots = np.cumsum([0] + [mf + 1 for _, _, mf in cases])
    d_off, d_len = up(filled(slots[-1], np.uint64)), up(filled(slots[-1], np.uint32))
    d_n, d_tail = up(filled(len(cases), np.uint32)), up(filled(len(cases), np.uint64))
    d_work = B.DeviceBuffer(B.wire_frames_launch_work(max(len(s) for s, _, _ in cases)) + 16)
    for k, (s, phase, mf) in enumerate(cases):
        assert (d_arena.ptr + at[k]) % 16 == phase
        B.wire_frames_launch(d_arena.ptr + at[k], len(s), d_off.ptr + 8 * int(slots[k]) if mf else None,
                             d_len.ptr + 4 * int(slots[k]) if mf else None, mf, d_n.ptr + 4 * k, d_tail.ptr + 8 * k,
                             d_work)
    H.synchronize()
    off, ln = d_off.download(dtype=np.uint64), d_len.download(dtype=np.uint32)
    n, tail = d_n.download(dtype=np.uint32), d_tail.download(dtype=np.uint64)
    for k, (s, phase, mf) in enumerate(cases):
        frames, t = M.split(s)
        kept = min(len(frames), mf)
        what = (k, len(s), phase, mf)
        want_off, want_len = filled(mf + 1, np.uint64), filled(mf + 1, np.uint32)
        want_off[:kept] = [f[0] for f in frames[:kept]]
        want_len[:kept] = [f[1] for f in frames[:kept]]
        assert off[slots[k]:slots[k + 1]].tolist() == want_off.tolist(), what
        assert ln[slots[k]:slots[k + 1]].tolist() == want_len.tolist(), what
        if len(s):
            assert (n[k], tail[k]) == (len(frames), t), what
        else:
            assert (n[k], tail[k]) == (EE32, EE64), what
    for b in (d_arena, d_off, d_len, d_n, d_tail, d_work):
        b.free()


def test_split_short_streams_and_the_three_tails():
    run_splits([(s, 0, 4) for s in (b"\n", b"x", b"", b"\nab", b"ab\n", b"a\n\nb", b"abc", b"\n\n", b"ab\ncd\nef")])


def test_split_every_phase_and_length():
    rng = np.random.default_rng(1)
    cases = []
    for phase in range(16):
        for n in range(1, 49):
            s = bytes(rng.choice(np.frombuffer(b"\nab", np.uint8), n, p=[0.3, 0.35, 0.35]))
            cases.append((s, phase, 49))
    cases += [(b"\n" * 48, p, 49) for p in range(16)] + [(b"x" * 48, p, 49) for p in range(16)]
    run_splits(cases)


@pytest.mark.parametrize("phase", [0, 1, 15])
def test_split_block_edges(phase):
    edge = BLOCK - phase  # the first byte of the second split block
    both = bytearray(b"x" * (2 * BLOCK))
    both[edge - 1] = both[edge] = 10
    last_only, first_only = bytearray(b"x" * (2 * BLOCK)), bytearray(b"x" * (2 * BLOCK))
    last_only[edge - 1] = first_only[edge] = 10
    solid = b"x" * edge + b"\n" * BLOCK + b"y" * BLOCK + b"\n"
    run_splits([(bytes(both), phase, 4), (bytes(last_only), phase, 4), (bytes(first_only), phase, 4),
                (solid, phase, BLOCK + 2), (bytes(both[:edge]), phase, 4), (bytes(both[:edge + 1]), phase, 4)])


def test_split_past_one_trip_of_the_scan():
    n = (SCAN + 1) * BLOCK - 7 - 100
    s = bytearray(b"x" * n)
    s[5] = s[n - 3] = 10
    assert (7 + n - 3) // BLOCK == SCAN
    run_splits([(bytes(s), 7, 4)])


def test_split_max_frames_below_at_and_zero():
    s = b"a\nbb\n\nccc\nd"
    run_splits([(s, 3, mf) for mf in (0, 1, 3, 4, 5, 9)])


def test_split_refuses_tables_that_do_not_fit():
    d = B.DeviceBuffer(4096)
    small = B.DeviceBuffer(16)
    with pytest.raises(B.LbfError, match="frame_offsets"):
        B.wire_frames_launch(d, 64, small, d, 3, d, d.ptr + 8, d.ptr + 64)
    with pytest.raises(B.LbfError, match="work"):
        B.wire_frames_launch(d, 4096, d, d, 3, d, d.ptr + 8, small.ptr + 12)
    with pytest.raises(B.LbfError, match="stream"):
        B.wire_frames_launch(small, 17, d, d, 3, d, d.ptr + 8, d.ptr + 64)
    d.free()
    small.free()


# ---- locate and bind -------------------------------------------------------
def run_locate(stream, table, files=None, max_chunks=0, live=None, phase=0, expected=None):
    """One launch over frame table `table` = [(offset, length)] of `stream`, placed at `phase`; d_frames, the dense
    tables and n_located compared whole with the model.  Returns the model's (frames, chunks)."""
    n = len(table)
    d_stream = up(np.frombuffer(b"\n" * (16 + phase) + stream + b"<", np.uint8))
    sp = d_stream.ptr + 16 + phase
    d_off, d_len = up(np.array([t[0] for t in table], np.uint64)), up(np.array([t[1] for t in table], np.uint32))
    d_frames = up(filled(n + 1, FD))
    d_work = B.DeviceBuffer(B.wire_send_chunks_launch_work(n) + 16)
    d_live = up(np.array([live], np.uint32)) if live is not None else None
    kw, bufs = {}, [d_stream, d_off, d_len, d_frames, d_work]
    mt = None
    if files is not None:
        mt = M.flood_table(files)
        t = B.wire_flood_table(files)
        dt = [up(a) for a in t]
        bufs += dt
        kw.update(file_names=dt[0], file_name_offsets=dt[1], file_first=dt[2], n_files=len(files), chunk_sizes=dt[3],
                  chunk_expected=dt[4], n_chunks=len(t[3]))
    if max_chunks:
        dense = [up(filled(max_chunks + 1, np.uint64)), up(filled(max_chunks + 1, np.uint32)),
                 up(filled(max_chunks + 1, np.uint32)), up(filled(20 * (max_chunks + 1), np.uint8)),
                 up(filled(max_chunks + 1, np.uint32)), up(filled(max_chunks + 1, np.uint32)),
                 up(filled(1, np.uint32))]
        bufs += dense
        kw.update(text_offsets=dense[0], text_lens=dense[1], expected_sizes=dense[2], expected=dense[3],
                  chunk_of=dense[4], frame_of=dense[5], max_chunks=max_chunks, n_located=dense[6])
    B.wire_send_chunks_launch(sp, len(stream), d_off, d_len, n, d_frames, d_work, live_frames=d_live, **kw)
    H.synchronize()
    n_live = n if live is None else min(live, n)
    if expected is None:
        expected = M.frames_expected(stream, table[:n_live], mt, FD)
    want, chunks = expected
    got = d_frames.download(dtype=FD)
    bad = np.nonzero(got[:n_live] != want)[0]
    assert bad.size == 0, (bad[:5], got[bad[0]], want[bad[0]], table[bad[0]])
    assert got[n_live:].tobytes() == filled(n + 1 - n_live, FD).tobytes()
    if max_chunks:
        toff, tlen, size, exp, cof, fof, located = M.dense_expected(want, chunks, mt or ([], [0], [0], [], []),
                                                                    max_chunks)
        dtypes = (np.uint64, np.uint32, np.uint32, np.uint8, np.uint32, np.uint32)
        fills = (0xEE,) * 6  # not 0xFF for the two index tables: a neutral entry must be seen to be written
        for k, (model, dtype, fill) in enumerate(zip((toff, tlen, size, exp, cof, fof), dtypes, fills)):
            per = 20 if k == 3 else 1
            have = dense[k].download(dtype=dtype)[:per * (max_chunks + 1)]
            assert have[:per * max_chunks].tolist() == model.tolist(), k
            assert have[per * max_chunks:].tobytes() == filled(per, dtype, fill).tobytes(), k
        assert dense[6].download(dtype=np.uint32)[0] == located
    for b in bufs + ([d_live] if d_live else []):
        b.free()
    return want, chunks


def as_stream(frames):
    """The frames behind one another, each with its delimiter, and their table."""
    stream = b"".join(f + b"\n" for f in frames)
    table, tail = M.split(stream)
    assert tail == len(stream) and [stream[a:a + n] for a, n in table] == list(frames)
    return stream, table


@pytest.mark.parametrize("phase", [0, 5, 15])
def test_locate_the_hand_built_frames(phase):
    cases = M.hand_built_frames(TRIP)
    stream, table = as_stream([f for _, f in cases])
    want, _ = run_locate(stream, table, phase=phase)
    kinds = dict(zip((label for label, _ in cases), want["kind"]))
    assert kinds["size 0"] == kinds["name amp"] == kinds["spaced"] == kinds["< is the last byte"] == M.UNBOUND
    assert kinds["RequestChunk"] == kinds["empty"] == kinds["SendChunkX"] == kinds["missing /i4"] == M.OTHER
    long_text = want[[label for label, _ in cases].index("size %d" % ((2 * TRIP + 1) * 3 // 4 + 3))]["text_len"]
    assert long_text > 2 * TRIP + 1


def test_locate_every_prefix_of_a_frame_with_its_completion_behind_it():
    frame = M.encode_send_chunk(b"a&b", 12, b"\x01\x02\x03\x04")
    want, _ = run_locate(frame, [(0, k) for k in range(len(frame))], phase=3)
    assert want["kind"].tolist() == [M.UNBOUND if k > frame.index(b"</base64>") else M.OTHER
                                     for k in range(len(frame))]


def test_locate_the_needle_at_every_lane_and_trip_boundary():
    base = M.encode_send_chunk(b"f", 9, b"abcdefg")[:-1]
    pad = (b"<methodNam" * (2 * TRIP // 10 + 3))  # decoys: every '<' is checked against the needle
    frames = [(pad[:j] if j % 3 else b"x" * j) + base for j in range(2 * TRIP + 14)]
    stream, table = as_stream(frames)
    loc = M.locate(base)
    want = np.zeros(len(frames), FD)
    for j, (at, _) in enumerate(table):
        want[j] = (at + j + loc["text_off"], at + j + loc["name_off"], loc["text_len"], loc["name_len"], 9, M.UNBOUND)
    for j in (0, 1, 15, 16, TRIP - 1, TRIP, 2 * TRIP + 13):  # the shortcut above is the model
        assert M.frames_expected(stream, [table[j]], None, FD)[0][0] == want[j]
    run_locate(stream, table, expected=(want, [None] * len(frames)))


def test_locate_the_text_ends_at_the_frames_last_byte_or_not_at_all():
    cut = M.encode_send_chunk(b"f", 1, b"xyz")[:-1]
    cut = cut[:cut.index(b"</base64>")]
    stream = cut + b"<" + b"\n" + cut  # run_locate puts a '<' directly behind the stream
    want, _ = run_locate(stream, [(0, len(cut) + 1), (0, len(cut)), (len(cut) + 2, len(cut))])
    assert want["kind"].tolist() == [M.UNBOUND, M.OTHER, M.OTHER]


def test_locate_frames_outside_the_stream_are_not_read():
    f = M.encode_send_chunk(b"f", 1, b"xyz")[:-1]
    want, _ = run_locate(f, [(0, len(f)), (1, len(f)), (len(f), 0), (len(f) + 1, 0), (1 << 40, 5), (0, 0xFFFFFFFF)])
    assert want["kind"].tolist() == [M.UNBOUND] + [M.OTHER] * 5


FILES = [(b"ab", [10, 11, 12], [M.sha1(b"ab%d" % k) for k in range(3)]),
         (b"abc", [20, 21], [M.sha1(b"abc%d" % k) for k in range(2)]),
         (b"a&b<", [30], [M.sha1(b"amp")])]


def bind_frames():
    enc = lambda name, i, **kw: M.send_chunk_text(name, i, b"QUJDRA==", **kw)[:-1]  # noqa: E731
    other = lambda n: n.replace(b"&", b"&#38;").replace(b"<", b"&lt;")  # noqa: E731  (not XmlEncode's form)
    return [enc(b"ab", 0), enc(b"abc", 1), enc(b"a&b<", 0), enc(b"a&b<", 0, escape=other), enc(b"nowhere", 0), enc(b"a", 0), enc(b"abcd", 0), enc(b"ab", 2), enc(b"ab", 3), enc(b"abc", 2),
            M.encode_method(b"RequestChunk", [b"ab", 1])[:-1], enc(b"ab", 0), b"", enc(b"ab", 0xFFFFFFFF),
            enc(b"ab", 0, idx=b"4294967296")]


@pytest.mark.parametrize("max_chunks", [0, 1, 5, 6, 7, 20])
def test_bind_and_the_dense_tables(max_chunks):
    stream, table = as_stream(bind_frames())
    want, chunks = run_locate(stream, table, files=FILES, max_chunks=max_chunks, phase=9)
    assert chunks == [0, 4, 5, None, None, None, None, 2, None, None, None, 0, None, None, 0]
    assert sum(c is not None for c in chunks) == 6


def test_bind_without_a_flood_table_and_with_fewer_live_frames():
    stream, table = as_stream(bind_frames())
    want, chunks = run_locate(stream, table, files=None, max_chunks=3)
    assert chunks == [None] * len(table) and (want["kind"] != M.SEND_CHUNK).all()
    for live in (0, 1, 8, len(table), len(table) + 5):
        run_locate(stream, table, files=FILES, max_chunks=9, live=live)


def test_bind_no_frames_makes_the_dense_tables_neutral():
    run_locate(b"x", [], files=FILES, max_chunks=5)
    run_locate(b"x", [], files=None, max_chunks=5)


def test_bind_past_one_trip_of_the_scan():
    n = GROUP * SCAN + 1
    f = M.send_chunk_text(b"abc", 1, b"QUJDRA==")[:-1]
    where = [0, GROUP - 1, GROUP, 2 * GROUP - 1, GROUP * (SCAN - 1), GROUP * SCAN - 1, GROUP * SCAN]
    lens = np.zeros(n, np.int64)
    lens[where] = len(f)
    offs = np.concatenate([[0], np.cumsum(lens + 1)[:-1]])
    stream = bytearray(b"\n" * int(offs[-1] + lens[-1] + 1))
    for w in where:
        stream[int(offs[w]):int(offs[w]) + len(f)] = f
    table = list(zip(offs.tolist(), lens.tolist()))
    want = np.zeros(n, FD)
    part = M.frames_expected(bytes(stream), [table[w] for w in where], M.flood_table(FILES), FD)
    want[where] = part[0]
    chunks = [None] * n
    for w in where:
        chunks[w] = 4
    assert (want["kind"][where] == M.SEND_CHUNK).all()
    run_locate(bytes(stream), table, files=FILES, max_chunks=len(where) + 1, expected=(want, chunks))


def test_send_chunks_refuses_tables_that_do_not_fit():
    d, small = B.DeviceBuffer(4096), B.DeviceBuffer(16)
    with pytest.raises(B.LbfError, match="frames"):
        B.wire_send_chunks_launch(d, 64, d, d, 2, small, d.ptr + 1024)
    with pytest.raises(B.LbfError, match="work"):
        B.wire_send_chunks_launch(d, 64, d, d, 8, d.ptr + 1024, small)
    d.free()
    small.free()


# ---- the chain -------------------------------------------------------------
def chain_stream():
    rng = np.random.default_rng(11)
    data = {k: rng.integers(0, 256, n, dtype=np.uint8).tobytes() for k, n in
            enumerate((300, 299, 1, 0, 55, 300, 162))}
    files = [(b"one.bin", [300, 299, 1, 0], [M.sha1(data[k]) for k in range(4)]),
             (b"two&.bin", [55, 300, 162], [M.sha1(data[4]), M.sha1(b"another chunk"), M.sha1(data[6])])]
    damaged = bytearray(M.encode_send_chunk(b"one.bin", 1, data[1]))
    damaged[damaged.index(b"<base64>") + 8 + 100] = ord("*")
    frames = [M.encode_method(b"NotifyHaveChunk", [b"one.bin", 0]),
              M.encode_send_chunk(b"one.bin", 0, data[0]),         # the xmlrpc++ layout
              M.encode_send_chunk_flat(b"two&.bin", 2, data[6]),   # a Java / Perl peer's
              bytes(damaged),
              M.encode_send_chunk(b"two&.bin", 1, data[5]),        # the table holds another hash
              M.encode_send_chunk(b"three.bin", 0, data[0]),       # not in the flood
              M.encode_method(b"RequestChunk", [b"two&.bin", 1]), b"\n",
              M.encode_send_chunk_flat(b"one.bin", 2, data[2]), M.encode_send_chunk(b"one.bin", 3, data[3]),
              M.encode_send_chunk(b"two&.bin", 0, data[4]), M.encode_send_chunk_flat(b"one.bin", 0, data[0])]
    unfinished = M.encode_send_chunk(b"one.bin", 1, data[1])[:200]
    return b"".join(frames) + unfinished, files, data, len(b"".join(frames))


def test_the_chain_from_a_raw_stream_to_verdicts_with_no_host_step():
    stream, files, data, tail_at = chain_stream()
    table, tail = M.split(stream)
    assert tail == tail_at
    mt = M.flood_table(files)
    max_frames, max_chunks, slot, max_text = 16, 10, 304, 512
    want_frames, chunks = M.frames_expected(stream, table, mt, FD)
    toff, tlen, size, exp, cof, fof, located = M.dense_expected(want_frames, chunks, mt, max_chunks)
    assert cof[:located].tolist() == [0, 6, 1, 5, 2, 3, 4, 0] and located < max_chunks

    phase = 7
    d_stream = up(np.frombuffer(b"\n" * (16 + phase) + stream + b"\n", np.uint8))
    sp = d_stream.ptr + 16 + phase
    d_off, d_len = up(filled(max_frames, np.uint64)), up(filled(max_frames, np.uint32))
    d_n, d_tail = up(filled(1, np.uint32)), up(filled(1, np.uint64))
    d_frames = up(filled(max_frames, FD))
    dt = [up(a) for a in B.wire_flood_table(files)]
    dense = [up(filled(max_chunks * per, dtype)) for per, dtype in ((1, np.uint64), (1, np.uint32), (1, np.uint32),
                                                                    (20, np.uint8), (1, np.uint32), (1, np.uint32))]
    dense.append(up(filled(1, np.uint32)))
    d_w1 = B.DeviceBuffer(B.wire_frames_launch_work(len(stream)))
    d_w2 = B.DeviceBuffer(B.wire_send_chunks_launch_work(max_frames))
    d_w3 = B.DeviceBuffer(max(B.b64_verify_launch_work(max_chunks), 16))
    d_out = up(filled(slot * max_chunks, np.uint8))
    d_out_off = up(np.arange(max_chunks, dtype=np.uint64) * slot)
    d_out_sizes, d_verdicts = up(filled(max_chunks, np.uint32)), up(filled(max_chunks, np.uint8))
    lib = B._capi.load()
    st = B._capi.ctypes.c_void_p()
    B._capi.check(lib.lbf_stream_create(B._capi.ctypes.byref(st)))
    try:
        B.wire_frames_launch(sp, len(stream), d_off, d_len, max_frames, d_n, d_tail, d_w1, stream=st)
        B.wire_send_chunks_launch(sp, len(stream), d_off, d_len, max_frames, d_frames, d_w2, live_frames=d_n,
                                  file_names=dt[0], file_name_offsets=dt[1], file_first=dt[2], n_files=len(files),
                                  chunk_sizes=dt[3], chunk_expected=dt[4], n_chunks=len(mt[3]), text_offsets=dense[0],
                                  text_lens=dense[1], expected_sizes=dense[2], expected=dense[3], chunk_of=dense[4],
                                  frame_of=dense[5], max_chunks=max_chunks, n_located=dense[6], stream=st)
        B.verify_b64_launch(sp, dense[0], dense[1], max_chunks, max_text, dense[2], slot, d_out, d_out_off, d_out_sizes,
                            d_w3, expected=dense[3], verdicts=d_verdicts, stream=st)
        B._capi.check(lib.lbf_stream_synchronize(st))
    finally:
        B._capi.check(lib.lbf_stream_destroy(st))
    assert d_n.download(dtype=np.uint32)[0] == len(table) and d_tail.download(dtype=np.uint64)[0] == tail_at
    got = d_frames.download(dtype=FD)
    assert got[:len(table)].tolist() == want_frames.tolist()
    assert got[len(table):].tobytes() == filled(max_frames - len(table), FD).tobytes()
    for have, model, dtype in zip(dense, (toff, tlen, size, exp, cof, fof), (np.uint64, np.uint32, np.uint32, np.uint8,
                                                                             np.uint32, np.uint32)):
        assert have.download(dtype=dtype)[:model.size].tolist() == model.tolist()
    assert dense[6].download(dtype=np.uint32)[0] == located
    verdicts = d_verdicts.download(dtype=np.uint8)[:max_chunks]
    # frames 1, 2, 8, 9, 10, 11 carry a chunk whole; the damaged text and the wrong hash fail; neutral entries fail
    assert verdicts.tolist() == [1, 1, 0, 0, 1, 1, 1, 1, 0, 0]
    out, sizes = d_out.download(), d_out_sizes.download(dtype=np.uint32)
    for j in range(located):
        if verdicts[j]:
            c = int(cof[j])
            assert sizes[j] == len(data[c]) and out[slot * j:slot * j + sizes[j]].tobytes() == data[c], j
    for b in [d_stream, d_off, d_len, d_n, d_tail, d_frames, d_w1, d_w2, d_w3, d_out, d_out_off, d_out_sizes,
              d_verdicts] + dt + dense:
        b.free()


def test_the_chain_with_the_cxx_side_as_the_judge(tmp_path):
    """tests/c/wire_chain_judge.cpp: frames by PeerWire::EncodeSendChunk, the table by Flood::WireTable, the two
    launches, every lbf_wire_frame against PeerWire::LocateSendChunk."""
    exe = build_program(tmp_path, "wire_chain_judge.cpp", "wire_chain_judge")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1].startswith("wire_chain_judge: OK"), r.stdout[-3000:]

#!/usr/bin/env python3
"""What a device-resident receive costs in front of the decode: the two launches
lbf_wire_frames_launch and lbf_wire_send_chunks_launch alone and in the chain
stream -> verdicts, against lbf_b64_verify_launch alone on tables the host made
beforehand (diagnostic, not the bench; recorded in DESIGN.md §4.11 and §5, not
gated).

C5's shape: `--frames` (1,024) SendChunk frames of `--chunk` (256 KiB) chunks in
the xmlrpc++ text layout, back to back in one stream in HBM.  One process
alternates, round by round,
  split      lbf_wire_frames_launch
  locate     lbf_wire_send_chunks_launch with the flood table and the dense tables
  verify     lbf_b64_verify_launch on tables uploaded from the host
  chain      the three behind one another, the decode reading the tables the
             second launch wrote
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` passes per figure.  A case's spread is its
max - min over the rounds; added_by_the_launches_us is chain's median minus
verify's, to be read next to verify's own spread.  hbm_frac counts the bytes a
case must read at least (the stream for the split, the stream again for the
locate) against the HBM peak bench.py's roofline uses.

For scale, host_one_core_us: memchr over the same stream and
PeerWire::LocateSendChunk on every frame, on one core, timed by a small program
this tool compiles against libbitflood.so (tools/wire_host_rate.cpp).

In the warm-up the results must be the CPU's: the frame table is the host
split's, every frame is bound to its chunk, every verdict is 1.

Run it under a time limit:
  timeout -k 10 900 python tools/wire_frames_rate.py --out profiles/wire_frames/rate.json
"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import signal
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bitflood_amd as B  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import LIB_PATH, check, load  # noqa: E402

HBM_PEAK_GBS = 8000.0  # bench.py's roofline constant


def build_stream(frames, chunk, seed):
    """(stream, [digest], name): EncodeSendChunk's bytes for `frames` chunks of one file."""
    rng = np.random.default_rng(seed)
    name = b"payload.bin"
    parts, digests = [], []
    for k in range(frames):
        data = rng.bytes(chunk)
        digests.append(hashlib.sha1(data).digest())
        text = base64.b64encode(data)
        lines = [text[i:i + 72] for i in range(0, len(text), 72)]
        body = b" ".join(lines) + (b" " if chunk % 54 == 0 and chunk else b"")
        parts.append(b'<?xml version="1.0"?>  <methodCall><methodName>SendChunk</methodName>  <params><param><value>' +
                     name + b"</value></param><param><value><i4>%d</i4></value></param><param><value><base64>" % k +
                     body + b"</base64></value></param></params></methodCall>  \n")
    return b"".join(parts), digests, name


def host_leg(stream_path, n_frames):
    """One core: memchr split + LocateSendChunk over the stream, microseconds (median of 5), by a program built here."""
    libdir = os.path.dirname(LIB_PATH)
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "wire_host_rate")
        subprocess.run(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tools", "wire_host_rate.cpp"), "-o", exe, "-L" + libdir, "-lbitflood",
                        "-llbfhash", "-Wl,-rpath," + libdir, "-lpthread"], check=True)
        out = subprocess.run([exe, stream_path], capture_output=True, text=True, check=True, timeout=300).stdout.split()
    assert int(out[0]) == n_frames and int(out[1]) == n_frames, out
    return float(out[2])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=1024)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4)
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = load()
    torch.cuda.set_device(0)
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    bufs = {}
    try:
        n, size = a.frames, a.chunk
        text, digests, name = build_stream(n, size, 0x5EED)
        host = np.frombuffer(text, np.uint8)
        table = B.wire_flood_table([(name, [size] * n, digests)])
        frame_off, frame_len, text_off, text_len, start = [], [], [], [], 0
        for k in range(n):
            end = text.index(b"\n", start)
            t0 = text.index(b"<base64>", start) + 8
            frame_off.append(start), frame_len.append(end - start)
            text_off.append(t0), text_len.append(text.index(b"<", t0) - t0)
            start = end + 1
        max_text = max(text_len)

        def dev(key, arr=None, nbytes=0):
            bufs[key] = B.DeviceBuffer(max(nbytes if arr is None else np.asarray(arr).nbytes, 16))
            if arr is not None:
                bufs[key].upload(np.ascontiguousarray(arr).view(np.uint8).reshape(-1))
            return bufs[key]

        d_stream = dev("stream", host)
        d_tab = [dev("tab%d" % k, t) for k, t in enumerate(table)]
        d_off, d_len = dev("off", nbytes=8 * n), dev("len", nbytes=4 * n)
        d_n, d_tail, d_frames = dev("n", nbytes=4), dev("tail", nbytes=8), dev("frames", nbytes=32 * n)
        dense = [dev("d%d" % k, nbytes=b * n) for k, b in enumerate((8, 4, 4, 20, 4, 4))] + [dev("nloc", nbytes=4)]
        h_toff, h_tlen = dev("h_toff", np.array(text_off, np.uint64)), dev("h_tlen", np.array(text_len, np.uint32))
        h_esz, h_exp = dev("h_esz", table[3]), dev("h_exp", table[4])
        d_w1 = dev("w1", nbytes=B.wire_frames_launch_work(len(text)))
        d_w2 = dev("w2", nbytes=B.wire_send_chunks_launch_work(n))
        d_w3 = dev("w3", nbytes=B.b64_verify_launch_work(n))
        d_out = dev("out", nbytes=n * size)
        d_out_off = dev("out_off", np.arange(n, dtype=np.uint64) * np.uint64(size))
        d_sizes, d_ver = dev("sizes", nbytes=4 * n), dev("ver", nbytes=n)

        def split():
            B.wire_frames_launch(d_stream, len(text), d_off, d_len, n, d_n, d_tail, d_w1, stream=sp)

        def locate():
            B.wire_send_chunks_launch(d_stream, len(text), d_off, d_len, n, d_frames, d_w2, live_frames=d_n,
                                      file_names=d_tab[0], file_name_offsets=d_tab[1], file_first=d_tab[2], n_files=1,
                                      chunk_sizes=d_tab[3], chunk_expected=d_tab[4], n_chunks=n, text_offsets=dense[0],
                                      text_lens=dense[1], expected_sizes=dense[2], expected=dense[3], chunk_of=dense[4],
                                      frame_of=dense[5], max_chunks=n, n_located=dense[6], stream=sp)

        def verify(toff, tlen, esz, exp):
            def run():
                B.verify_b64_launch(d_stream, toff, tlen, n, max_text, esz, size, d_out, d_out_off, d_sizes, d_w3,
                                    expected=exp, verdicts=d_ver, stream=sp)
            return run

        verify_host, verify_dev = verify(h_toff, h_tlen, h_esz, h_exp), verify(dense[0], dense[1], dense[2], dense[3])

        def chain():
            split(), locate(), verify_dev()

        def verdicts_ok():
            return bool((d_ver.download(n) == 1).all())

        def split_ok():
            return (int(d_n.download(4, dtype=np.uint32)[0]) == n and int(d_tail.download(8, dtype=np.uint64)[0]) ==
                    len(text) and d_off.download(8 * n, dtype=np.uint64).tolist() == frame_off and
                    d_len.download(4 * n, dtype=np.uint32).tolist() == frame_len)

        def locate_ok():
            return (int(dense[6].download(4, dtype=np.uint32)[0]) == n and
                    dense[0].download(8 * n, dtype=np.uint64).tolist() == text_off and
                    dense[1].download(4 * n, dtype=np.uint32).tolist() == text_len and
                    dense[4].download(4 * n, dtype=np.uint32).tolist() == list(range(n)) and
                    bool((d_frames.download(32 * n, dtype=H.WIRE_FRAME_DTYPE)["kind"] == 1).all()))

        def clear():
            d_ver.upload(np.zeros(n, np.uint8))

        cases = [("split", split, split_ok), ("locate", locate, locate_ok), ("verify", verify_host, verdicts_ok),
                 ("chain", chain, lambda: split_ok() and locate_ok() and verdicts_ok())]

        def timed(fn, reps):
            signal.alarm(a.step_timeout)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            signal.alarm(0)
            return e0.elapsed_time(e1) * 1000.0 / reps  # us a pass

        us, agree = {}, {}
        for name_, fn, ok in cases:  # warm-up, and every case's results
            clear()
            timed(fn, 1)
            agree[name_], us[name_] = bool(ok()), []
        for _ in range(a.rounds):
            for name_, fn, _ in cases:
                us[name_].append(timed(fn, a.reps))
        with tempfile.NamedTemporaryFile(suffix=".stream") as f:
            f.write(text)
            f.flush()
            host_us = host_leg(f.name, n)
        res = {"mode": "wire-frames-rate", "frames": n, "chunk": size, "stream_bytes": len(text), "rounds": a.rounds,
               "reps": a.reps, "hbm_peak_gbs": HBM_PEAK_GBS, "tuned": False, "cases": {}}
        for name_, v in us.items():
            med = statistics.median(v)
            res["cases"][name_] = {"us_median": round(med, 2), "us_min": round(min(v), 2), "us_max": round(max(v), 2),
                                   "spread_us": round(max(v) - min(v), 2), "results_agree": agree[name_]}
            if name_ in ("split", "locate"):
                res["cases"][name_]["hbm_frac"] = round(len(text) / (med * 1e-6) / 1e9 / HBM_PEAK_GBS, 4)
        res["added_by_the_launches_us"] = round(res["cases"]["chain"]["us_median"] -
                                                res["cases"]["verify"]["us_median"], 2)
        res["verify_spread_us"] = res["cases"]["verify"]["spread_us"]
        res["host_one_core_us"] = round(host_us, 1)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if all(agree.values()) else 1
    finally:
        for b in bufs.values():
            b.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

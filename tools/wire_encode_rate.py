#!/usr/bin/env python3
"""Rate of the piecewise base64 encode beside the resumable SHA-1
(lbf_b64_encode_update_launch), device-resident (diagnostic, not the bench;
recorded in DESIGN.md §4.8 and §5, not gated).

C2's shape in HBM: 16,384 chunks of 256 KiB (lbf_fill_synthetic), each with a
text slot of its own.  One process alternates, round by round,
  e1_xmlrpc, e1_flat   the chunk as one piece with the final flag, through the
                       new launch (three enqueues: sizes, hash, encode), in
                       xmlrpc++'s lines and unbroken
  e4_*, e64_*          4 and 64 pieces of a quarter / a 64th of the chunk each
  h1, h4, h64          lbf_sha1_update_launch alone on the same pieces
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` passes per figure; e - h is the encode's share,
and a case's spread is its max - min over the rounds.  After the warm-up every
verdict must be 1, every text length the chunk's, and the text of the first
`--probe-chunks` chunks what base64 gives on the host.

With --one-shot the cases are those of the one-shot wire encode
(lbf_verify_encode_b64_launch), alternating in the same way:
  k_xmlrpc, k_flat     `--kernel-chunks` (1,024) chunks, no hash: the line kernel
                       (b64_encode_kernel) alone and the flat kernel
                       (b64_flat_encode_kernel) alone on the same bytes
  o_xmlrpc, o_flat     C2's shape, the one-shot launch: hash, encode, verdicts
  e1_xmlrpc, e1_flat   the piecewise launch with one final piece per chunk
  s1                   lbf_sha1_launch alone on the same table: the floor
and the same checks after the warm-up.

Run it under a time limit:
  timeout -k 10 600 python tools/wire_encode_rate.py --out profiles/b64_encode_update/wire_encode_rate.json
  timeout -k 10 600 python tools/wire_encode_rate.py --one-shot --out profiles/b64_flat_encode/one_shot.json
"""
import argparse
import base64
import ctypes
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bitflood_amd import DeviceBuffer, b64_text_length, new_b64_enc_states, new_states  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import check, load  # noqa: E402

LAYOUTS = ("xmlrpc", "flat")


def host_text(chunk: np.ndarray, layout: str) -> bytes:
    s = base64.b64encode(chunk)
    if layout == "flat":
        return s
    lines = chunk.size // 3 // 18
    return b"".join(s[72 * k:72 * k + 72] + b" " for k in range(lines)) + s[72 * lines:]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="passes per case per round")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--probe-chunks", type=int, default=64, help="chunks whose text is compared with the host's")
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases (for a counter run of one)")
    ap.add_argument("--one-shot", action="store_true", help="the one-shot launch against the piecewise one")
    ap.add_argument("--kernel-chunks", type=int, default=1024, help="--one-shot: chunks of the encode-only cases")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, cs = a.chains, a.chunk
    lib = load()
    torch.cuda.set_device(0)
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    tl = {lay: b64_text_length(cs, lay) for lay in LAYOUTS}
    slot = (max(tl.values()) + 15) // 16 * 16  # every slot 16-byte aligned, as a sender's frame buffer would be
    parts = (1,) if a.one_shot else (1, 4, 64)
    b = dict(data=DeviceBuffer(n * cs), ref=DeviceBuffer(20 * n), dig=DeviceBuffer(20 * n), sha=DeviceBuffer(96 * n),
             fin1=DeviceBuffer(n), fin0=DeviceBuffer(n), ver=DeviceBuffer(n), text=DeviceBuffer(n * slot),
             toff=DeviceBuffer(8 * n), noff=DeviceBuffer(8 * n), nlen=DeviceBuffer(4 * n), tsz=DeviceBuffer(4 * n))
    try:
        b["data"].fill_synthetic(0x5EED)
        b["sha"].upload(new_states(n))
        b["fin1"].upload(np.ones(n, dtype=np.uint8))
        b["fin0"].upload(np.zeros(n, dtype=np.uint8))
        H.set_kernel_variant(0)
        H.uniform_launch(b["data"], n * cs, cs, 0, n, b["ref"])
        H.synchronize()
        want = b["ref"].download(20 * n).tobytes()
        base = np.arange(n, dtype=np.uint64)
        b["toff"].upload(base * np.uint64(slot))
        for lay in LAYOUTS:
            b["enc", lay], b["caps", lay] = DeviceBuffer(16 * n), DeviceBuffer(4 * n)
            b["enc", lay].upload(new_b64_enc_states(n, lay))
            b["caps", lay].upload(np.full(n, tl[lay], dtype=np.uint32))
        for p in parts:  # the chunk's bytes in p equal parts
            b["size", p] = DeviceBuffer(4 * n)
            b["size", p].upload(np.full(n, cs // p, dtype=np.uint32))
            for k in range(p):
                b["off", p, k] = DeviceBuffer(8 * n)
                b["off", p, k].upload(base * np.uint64(cs) + np.uint64(k * (cs // p)))

        def encode_pieces(p, lay):
            def run():
                for k in range(p):
                    H.b64_encode_update_launch(b["enc", lay], b["sha"], n, None, b["data"], b["off", p, k],
                                               b["size", p], b["fin1"] if k == p - 1 else b["fin0"], n, b["text"],
                                               b["toff"], b["caps", lay], b["noff"], b["nlen"], b["tsz"], b["dig"],
                                               b["ref"], b["ver"], stream=sp)
            return run

        def hash_pieces(p):
            def run():
                for k in range(p):
                    H.update_launch(b["sha"], n, None, b["data"], b["off", p, k], b["size", p],
                                    b["fin1"] if k == p - 1 else b["fin0"], n, b["dig"], b["ref"], b["ver"], stream=sp)
            return run

        def one_shot(lay, chunks, hashed):
            def run():
                H.verify_encode_b64_launch(b["data"], b["off", 1, 0], b["size", 1], chunks, cs, b["text"], b["toff"],
                                           layout=lay, digests=b["dig"] if hashed else None,
                                           expected=b["ref"] if hashed else None,
                                           verdicts=b["ver"] if hashed else None, stream=sp)
            return run

        def hash_alone():
            H.batch_launch(b["data"], b["off", 1, 0], b["size", 1], n, b["dig"], b["ref"], b["ver"], stream=sp)

        # (name, launch, calls per pass, layout of the text or None, chunks hashed, chunks in all, sets text sizes)
        if a.one_shot:
            k = min(a.kernel_chunks, n)
            cases = [(f"k_{lay}", one_shot(lay, k, False), 1, lay, 0, k, False) for lay in LAYOUTS]
            cases += [(f"o_{lay}", one_shot(lay, n, True), 1, lay, n, n, False) for lay in LAYOUTS]
            cases += [(f"e1_{lay}", encode_pieces(1, lay), 1, lay, n, n, True) for lay in LAYOUTS]
            cases += [("s1", hash_alone, 1, None, n, n, False)]
        else:
            cases = [(f"e{p}_{lay}", encode_pieces(p, lay), p, lay, n, n, True) for p in parts for lay in LAYOUTS]
            cases += [(f"h{p}", hash_pieces(p), p, None, n, n, False) for p in parts]
        if a.cases:
            keep = a.cases.split(",")
            cases = [c for c in cases if c[0] in keep or c[0].split("_")[0] in keep]
        ms = {name: [] for name, *_ in cases}
        agree = {}

        def timed(fn, reps):
            signal.alarm(a.step_timeout)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            signal.alarm(0)
            return e0.elapsed_time(e1) / reps

        m = min(a.probe_chunks, n)
        host = b["data"].download(m * cs)
        for name, fn, _, lay, hashed, chunks, sized in cases:  # warm-up, and every case's results
            b["dig"].upload(np.zeros(20 * n, dtype=np.uint8))
            b["ver"].upload(np.zeros(n, dtype=np.uint8))
            if lay:
                b["tsz"].upload(np.zeros(n, dtype=np.uint32))
                b["text"].upload(np.zeros(m * slot, dtype=np.uint8))
            timed(fn, 1)
            ok = hashed == 0 or (b["dig"].download(20 * hashed).tobytes() == want[:20 * hashed] and
                                 bool(b["ver"].download(hashed).all()))
            if lay:
                if sized:
                    ok = ok and bool((b["tsz"].download(4 * n, dtype=np.uint32) == tl[lay]).all())
                got = b["text"].download(m * slot)
                ok = ok and all(got[i * slot:i * slot + tl[lay]].tobytes() == host_text(host[i * cs:(i + 1) * cs], lay)
                                for i in range(m))
            agree[name] = ok
        for _ in range(a.rounds):
            for name, fn, *_ in cases:
                ms[name].append(timed(fn, a.reps))
        gib = n * cs / 2**30
        res = {"mode": "one-shot" if a.one_shot else "encode", "chains": n, "chunk": cs, "text_chars": tl,
               "gib_encoded": gib, "rounds": a.rounds, "reps": a.reps, "library": os.environ.get("LBF_LIB", "in-tree"),
               "cases": {}}
        for name, _, launches, _, _, chunks, _ in cases:
            v = ms[name]
            per = 4 / (chunks * cs / 2**30)  # a pass of this case's chunks -> 4 GiB
            res["cases"][name] = {"launches_per_pass": launches, "chunks": chunks,
                                  "us_per_pass_median": round(statistics.median(v) * 1000, 2),
                                  "us_per_pass_min": round(min(v) * 1000, 2),
                                  "us_per_pass_max": round(max(v) * 1000, 2),
                                  "ms_per_4gib_median": round(statistics.median(v) * per, 4),
                                  "ms_min": round(min(v) * per, 4), "ms_max": round(max(v) * per, 4),
                                  "spread_ms": round((max(v) - min(v)) * per, 4), "results_agree": agree[name]}
        if a.one_shot and not a.cases:
            med = {name: c["ms_per_4gib_median"] for name, c in res["cases"].items()}
            res["one_shot_minus_piecewise_ms"] = {lay: round(med[f"o_{lay}"] - med[f"e1_{lay}"], 4) for lay in LAYOUTS}
            res["encode_share_ms"] = {f"o_{lay}": round(med[f"o_{lay}"] - med["s1"], 4) for lay in LAYOUTS}
            res["flat_minus_line_kernel_us"] = round(res["cases"]["k_flat"]["us_per_pass_median"] -
                                                     res["cases"]["k_xmlrpc"]["us_per_pass_median"], 2)
        elif not a.cases:
            res["encode_share_ms"] = {f"e{p}_{lay}": round(res["cases"][f"e{p}_{lay}"]["ms_per_4gib_median"] -
                                                           res["cases"][f"h{p}"]["ms_per_4gib_median"], 4)
                                      for p in parts for lay in LAYOUTS}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if all(agree.values()) else 1
    finally:
        for buf in b.values():
            buf.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Rate of the device-resident one-shot decode + verify (lbf_b64_verify_launch),
against what a receiver with frames in HBM had before it (diagnostic, not the
bench; recorded in DESIGN.md §4.5 and §5, not gated).

C2's shape in HBM: 16,384 chunks of 256 KiB (lbf_fill_synthetic), their text
written by the device encode (lbf_verify_encode_b64_launch) in xmlrpc++'s lines
and unbroken, each text in a slot of its own.  One process alternates, round by
round,
  a_xmlrpc, a_flat           A: the new launch (memset, routed tile decode,
                             scan of the redo chunks, lbf_sha1_launch, finish)
  b_xmlrpc, b_flat           B: lbf_b64_update_launch with one final piece per
                             chunk, the process-wide switches as the library
                             defaults them (today's default route)
  bf_xmlrpc, bf_flat         B on the fused route (lbf_set_b64_fused), the line
                             and the flat stage both on
  c                          C: lbf_sha1_launch alone on the decoded bytes
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` passes per figure.  A - C is the decode's share;
a case's spread is its max - min over the rounds.  In the warm-up every route's
verdicts must be 1, every size the chunk's, every digest the hash of the bytes,
and the decoded bytes of the first `--probe-chunks` chunks the bytes that were
encoded; for A, redo must be 0 everywhere (no chunk fell to the scan).

The bar: A below B by more than B's own max - min over the rounds of this run.

Run it under a time limit:
  timeout -k 10 600 python tools/wire_verify_rate.py --out profiles/b64_verify_launch/one_shot.json
"""
import argparse
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

from bitflood_amd import DeviceBuffer, b64_text_length, b64_verify_launch_work, new_b64_states, new_states  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import check, load  # noqa: E402

LAYOUTS = ("xmlrpc", "flat")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="passes per case per round")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--probe-chunks", type=int, default=64, help="chunks whose bytes are compared with the encoded ones")
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases (for a counter run of one)")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, cs = a.chains, a.chunk
    lib = load()
    torch.cuda.set_device(0)
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    tl = {lay: b64_text_length(cs, lay) for lay in LAYOUTS}
    slot = (max(tl.values()) + 15) // 16 * 16  # every slot 16-byte aligned, as a receiver's frame buffer would be
    b = dict(data=DeviceBuffer(n * cs), out=DeviceBuffer(n * cs), ref=DeviceBuffer(20 * n), dig=DeviceBuffer(20 * n),
             ver=DeviceBuffer(n), osz=DeviceBuffer(4 * n), work=DeviceBuffer(b64_verify_launch_work(n)),
             doff=DeviceBuffer(8 * n), size=DeviceBuffer(4 * n), toff=DeviceBuffer(8 * n), fin=DeviceBuffer(n),
             b64=DeviceBuffer(16 * n), sha=DeviceBuffer(96 * n), poff=DeviceBuffer(8 * n), psz=DeviceBuffer(4 * n))
    defaults = None
    try:
        for lay in LAYOUTS:
            b["text", lay], b["tlen", lay] = DeviceBuffer(n * slot), DeviceBuffer(4 * n)
            b["tlen", lay].upload(np.full(n, tl[lay], dtype=np.uint32))
        b["data"].fill_synthetic(0x5EED)
        base = np.arange(n, dtype=np.uint64)
        b["doff"].upload(base * np.uint64(cs))
        b["toff"].upload(base * np.uint64(slot))
        b["size"].upload(np.full(n, cs, dtype=np.uint32))
        b["fin"].upload(np.ones(n, dtype=np.uint8))
        b["b64"].upload(new_b64_states(n))
        b["sha"].upload(new_states(n))
        H.set_kernel_variant(0)
        for lay in LAYOUTS:  # the texts, and the digests every route must find
            H.verify_encode_b64_launch(b["data"], b["doff"], b["size"], n, cs, b["text", lay], b["toff"], layout=lay,
                                       digests=b["ref"])
        H.synchronize()
        want = b["ref"].download(20 * n).tobytes()
        # the switches as the library defaults them (read back by setting and restoring)
        defaults = (H.set_b64_lines(True), H.set_b64_flat(True), H.set_b64_fused(False))
        H.set_b64_lines(defaults[0])
        H.set_b64_flat(defaults[1])

        def one_shot(lay):
            def run():
                H.verify_b64_launch(b["text", lay], b["toff"], b["tlen", lay], n, tl[lay], b["size"], cs, b["out"],
                                    b["doff"], b["osz"], b["work"], digests=b["dig"], expected=b["ref"],
                                    verdicts=b["ver"], stream=sp)
            return run

        def piecewise(lay, fused):
            def run():
                # process-wide switches, read when the launch is made: set per call, restored at the end
                H.set_b64_fused(fused)
                H.set_b64_lines(True if fused else defaults[0])
                H.set_b64_flat(True if fused else defaults[1])
                H.b64_update_launch(b["b64"], b["sha"], n, None, b["text", lay], b["toff"], b["tlen", lay], b["fin"], n,
                                    b["out"], b["doff"], b["size"], b["osz"], b["dig"], b["ref"], b["ver"], b["poff"],
                                    b["psz"], stream=sp)
            return run

        def hash_alone():
            H.batch_launch(b["out"], b["doff"], b["size"], n, b["dig"], b["ref"], b["ver"], stream=sp)

        # (name, launch, decodes)
        cases = [(f"a_{lay}", one_shot(lay), True) for lay in LAYOUTS]
        cases += [(f"b_{lay}", piecewise(lay, False), True) for lay in LAYOUTS]
        cases += [(f"bf_{lay}", piecewise(lay, True), True) for lay in LAYOUTS]
        cases += [("c", hash_alone, False)]
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
        for name, fn, decodes in cases:  # warm-up, and every case's results
            b["dig"].upload(np.zeros(20 * n, dtype=np.uint8))
            b["ver"].upload(np.zeros(n, dtype=np.uint8))
            if decodes:
                b["osz"].upload(np.zeros(n, dtype=np.uint32))
                b["out"].upload(np.full(m * cs, 0xEE, dtype=np.uint8))
                b["work"].upload(np.full(2 * n, 0xEE, dtype=np.uint8))
            timed(fn, 1)
            ok = b["dig"].download(20 * n).tobytes() == want and bool(b["ver"].download(n).all())
            if decodes:
                ok = ok and bool((b["osz"].download(4 * n, dtype=np.uint32) == cs).all())
                ok = ok and bool(np.array_equal(b["out"].download(m * cs), host))
            if name.startswith("a_"):
                ok = ok and not b["work"].download(2 * n).any()  # nothing over, nothing to the scan
            agree[name] = ok
        for _ in range(a.rounds):
            for name, fn, _ in cases:
                ms[name].append(timed(fn, a.reps))
        per = 4 / (n * cs / 2**30)  # a pass -> 4 GiB of decoded bytes
        res = {"mode": "verify-one-shot", "chains": n, "chunk": cs, "text_chars": tl, "gib_decoded": n * cs / 2**30,
               "rounds": a.rounds, "reps": a.reps, "library": os.environ.get("LBF_LIB", "in-tree"),
               "switch_defaults": {"lines": defaults[0], "flat": defaults[1], "fused": defaults[2]}, "cases": {}}
        for name, _, _ in cases:
            v = ms[name]
            res["cases"][name] = {"us_per_pass_median": round(statistics.median(v) * 1000, 2),
                                  "ms_per_4gib_median": round(statistics.median(v) * per, 4),
                                  "ms_min": round(min(v) * per, 4), "ms_max": round(max(v) * per, 4),
                                  "spread_ms": round((max(v) - min(v)) * per, 4), "results_agree": agree[name]}
        if not a.cases:
            c = res["cases"]
            med = {name: x["ms_per_4gib_median"] for name, x in c.items()}
            res["decode_share_ms"] = {f"a_{lay}": round(med[f"a_{lay}"] - med["c"], 4) for lay in LAYOUTS}
            res["a_minus_b_ms"] = {f"{bb}_{lay}": round(med[f"a_{lay}"] - med[f"{bb}_{lay}"], 4)
                                   for bb in ("b", "bf") for lay in LAYOUTS}
            # the bar: A's median below B's by more than B's own max - min over the rounds
            res["a_below_b_by_more_than_b_spread"] = {
                f"{bb}_{lay}": bool(med[f"{bb}_{lay}"] - med[f"a_{lay}"] > c[f"{bb}_{lay}"]["spread_ms"])
                for bb in ("b", "bf") for lay in LAYOUTS}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if all(agree.values()) else 1
    finally:
        if defaults is not None:
            H.set_b64_lines(defaults[0])
            H.set_b64_flat(defaults[1])
            H.set_b64_fused(defaults[2])
        for buf in b.values():
            buf.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Rate of the resumable-state kernel against the one-shot lane kernel
(diagnostic, not the bench; recorded in DESIGN.md §5, not gated).

C2's shape, device-resident (lbf_fill_synthetic): 4 GiB as 16,384 chains of
256 KiB.  One process alternates, round by round,
  a   the shipped lane kernel one-shot (lbf_set_kernel_variant(1), lbf_sha1_launch)
  b   lbf_sha1_update_launch, one 256 KiB piece + final
  c   4 pieces of 64 KiB (4 launches per chunk)
  d   64 pieces of 4 KiB (64 launches per chunk)
  a2  a again: the run-to-run spread that b - a is read against
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` (>= 20) passes per figure.  Afterwards every
case's digests are compared with the one-shot digests of the automatic kernel.
c and d carry the per-call cost (launch + the state round trip through HBM).

Run it under a time limit:
  timeout -k 10 600 python tools/update_rate.py --out profiles/update_rate.json
"""
import argparse
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bitflood_amd import DeviceBuffer, new_states  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import check, load  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="passes per case per round")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert a.rounds * a.reps >= 20, "at least 20 passes per figure"
    n, cs = a.chains, a.chunk
    lib = load()
    torch.cuda.set_device(0)
    import ctypes
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)

    data, dig, ref = DeviceBuffer(n * cs), DeviceBuffer(20 * n), DeviceBuffer(20 * n)
    states, fin1, fin0 = DeviceBuffer(96 * n), DeviceBuffer(n), DeviceBuffer(n)
    sizes = {p: DeviceBuffer(4 * n) for p in (1, 4, 64)}
    offs = {}
    try:
        data.fill_synthetic(0x5EED)
        states.upload(new_states(n))
        fin1.upload(np.ones(n, dtype=np.uint8))
        fin0.upload(np.zeros(n, dtype=np.uint8))
        for p in (1, 4, 64):
            sizes[p].upload(np.full(n, cs // p, dtype=np.uint32))
            for k in range(p):
                offs[p, k] = DeviceBuffer(8 * n)
                offs[p, k].upload(np.arange(n, dtype=np.uint64) * np.uint64(cs) + np.uint64(k * (cs // p)))
        H.set_kernel_variant(0)
        H.uniform_launch(data, n * cs, cs, 0, n, ref)
        H.synchronize()
        want = ref.download(20 * n).tobytes()

        def one_shot():
            H.batch_launch(data, offs[1, 0], sizes[1], n, dig, stream=sp)

        def pieces(p):
            def run():
                for k in range(p):
                    H.update_launch(states, n, None, data, offs[p, k], sizes[p], fin1 if k == p - 1 else fin0, n, dig,
                                    stream=sp)
            return run

        cases = [("a", one_shot, 1), ("b", pieces(1), 1), ("c", pieces(4), 4), ("d", pieces(64), 64),
                 ("a2", one_shot, 1)]
        ms = {name: [] for name, _, _ in cases}
        agree = {}

        def timed(name, fn, reps):
            H.set_kernel_variant(1 if name.startswith("a") else 0)
            signal.alarm(a.step_timeout)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            signal.alarm(0)
            return e0.elapsed_time(e1) / reps

        for name, fn, _ in cases:  # warm-up, and the digests of every case
            dig.upload(np.zeros(20 * n, dtype=np.uint8))
            timed(name, fn, 1)
            agree[name] = dig.download(20 * n).tobytes() == want
        for _ in range(a.rounds):
            for name, fn, _ in cases:
                ms[name].append(timed(name, fn, a.reps))
        H.set_kernel_variant(0)
        gib = n * cs / 2**30
        res = {"chains": n, "chunk": cs, "gib": gib, "rounds": a.rounds, "reps": a.reps, "cases": {}}
        for name, _, launches in cases:
            med = statistics.median(ms[name])
            res["cases"][name] = {"launches_per_pass": launches, "ms_median": round(med, 4),
                                  "ms_min": round(min(ms[name]), 4), "ms_max": round(max(ms[name]), 4),
                                  "GiB/s": round(gib / (med * 1e-3), 1), "digests_agree": agree[name]}
        am, a2m, bm = (res["cases"][k]["ms_median"] for k in ("a", "a2", "b"))
        res["a_vs_a2_spread_ms"] = round(abs(am - a2m), 4)
        res["b_minus_a_ms"] = round(bm - min(am, a2m), 4)
        res["per_launch_extra_ms"] = {k: round((res["cases"][k]["ms_median"] - bm) / (res["cases"][k]["launches_per_pass"] - 1), 4)
                                      for k in ("c", "d")}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if all(agree.values()) else 1
    finally:
        for b in [data, dig, ref, states, fin1, fin0, *sizes.values(), *offs.values()]:
            b.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Randomised fuzz of the piecewise calls and the one-shot wire launches
(diagnostic, not a test; a fixed slice of it runs as tests/test_gpu_piece_fuzz.py).

Each case is one scene of tests/piece_cases.py (its docstring says what is
drawn): chains hashed, decoded or encoded piece by piece through a route drawn
per call -- the host calls, the one-piece launches, the seq launches -- under
(lines, flat, fused) switches drawn per call, every call resuming the records
the call before it left; or one of the two one-shot wire launches.  After every
call every byte of the output arena, every table entry and every record is held
against the CPU models (tests/piece_driver.py).  Stops at the first mismatch and
prints the case seed (--seed S --cases 1 replays it).

Usage: python tools/fuzz_pieces.py [--seconds 60] [--seed 1000] [--cases N]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (first: one HIP runtime per process)

from bitflood_amd import ChunkHasher  # noqa: E402
from tests import piece_cases as P  # noqa: E402
from tests.piece_driver import run_scene  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=60)
    ap.add_argument("--seed", type=int, default=1000, help="the first case's seed; case k has seed + k")
    ap.add_argument("--cases", type=int, default=0)
    a = ap.parse_args()
    t0, cases, calls, per_family = time.time(), 0, 0, {}
    with ChunkHasher(device_mask=1) as h:
        seed = a.seed
        while (a.cases and cases < a.cases) or (not a.cases and time.time() - t0 < a.seconds):
            scene = P.case(seed)
            try:
                calls += run_scene(h, scene)
            except P.Mismatch as e:
                print(str(e), file=sys.stderr, flush=True)
                print(json.dumps({"all_ok": False, "seed": seed, "family": scene.family,
                                  "where": str(e).splitlines()[0]}), flush=True)
                sys.exit(1)
            per_family[scene.family] = per_family.get(scene.family, 0) + 1
            cases += 1
            seed += 1
            if cases % 100 == 0:
                print(f"{cases} cases ok ({time.time() - t0:.0f} s)", file=sys.stderr, flush=True)
    print(json.dumps({"all_ok": True, "cases": cases, "calls": calls, "first_seed": a.seed, "per_family": per_family,
                      "seconds": round(time.time() - t0, 1)}))


if __name__ == "__main__":
    main()

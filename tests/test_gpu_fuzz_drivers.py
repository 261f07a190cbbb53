"""The four older random drivers of tools/, started once each so that they
cannot rot: a fixed seed, a small deterministic case count, and --seconds large
enough not to bind.  Each is a fresh child process with a time limit of its
own; it must leave with status 0 and "all_ok" in its JSON line.  The open-ended
campaigns stay what they were: diagnostics run by hand.
"""
import json
import os
import signal
import subprocess
import sys

import pytest

from tests.test_piece_cases import FUZZ_GPU_CASES, FUZZ_GPU_SEED

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# (tool, seed, cases, the child's time limit in seconds).  tools/fuzz_gpu.py's seed and
# count meet all 15 (variant, mode) pairs: test_fuzz_gpu_seed_reaches_every_variant_in_every_mode.
DRIVERS = [
    ("fuzz_gpu.py", FUZZ_GPU_SEED, FUZZ_GPU_CASES, 120),
    ("fuzz_b64.py", 5, 24, 120),
    ("fuzz_host_paths.py", 5, 12, 180),
    ("fuzz_cli.py", 5, 4, 180),
]


@pytest.mark.parametrize("tool,seed,cases,limit", DRIVERS, ids=[d[0][:-3] for d in DRIVERS])
def test_driver_runs_clean(tool, seed, cases, limit):
    args = [sys.executable, os.path.join(ROOT, "tools", tool), "--seed", str(seed), "--cases", str(cases),
            "--seconds", "3600"]
    p = subprocess.run(args, capture_output=True, text=True, timeout=limit, cwd=ROOT)
    tail = (p.stdout[-2000:], p.stderr[-2000:])
    if p.returncode < 0:  # the child ended on a signal: say which, and start nothing again
        pytest.fail(f"{tool} ended on signal {signal.Signals(-p.returncode).name}: {tail}")
    assert p.returncode == 0, (tool, p.returncode, tail)
    lines = [x for x in p.stdout.splitlines() if x.startswith("{")]
    assert lines, tail
    out = json.loads(lines[-1])
    assert out.get("all_ok") is True and out["cases"] == cases, out
    if tool == "fuzz_gpu.py":
        assert len(out["per_variant_mode"]) == 15, out

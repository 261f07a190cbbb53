"""bench.py's plain run on the GPU: `--gpus 1 --steps K --warmup W` times K
launches and prints the headline line without the legs of --full, and
--dump-outputs writes what the last timed launch left in HBM.  A 256 MiB file
keeps it to seconds."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def test_plain_run_dumps_the_digests_of_the_timed_path(oracle, tmp_path):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBF_BENCH_FORM_GROUP")}
    args = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
            "--file-gib", "0.25", "--dump-outputs", str(tmp_path / "out")]
    p = subprocess.run(args, env=env, capture_output=True, text=True, timeout=120, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == 1 and out["steps"] == 3 and out["full"] is False
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["value"] > 0 and out["ms_per_step"] > 0
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 0.25) < 1e-3
    for k in ("cpu_baseline", "e2e_host_to_host_gibs", "e2e_registered", "other_configs", "parity", "digest_check"):
        assert k not in out, k
    cs, n = 262144, 1024
    data = oracle.synth(0x5EED, 0, n * cs, nthreads=8)
    want = oracle.sha1_batch(data, np.arange(n, dtype=np.uint64) * np.uint64(cs), np.full(n, cs, np.uint32),
                             nthreads=8)
    got = np.load(tmp_path / "out" / "digests.npy")
    assert got.dtype == np.float32 and got.shape == (n, 20)
    assert np.array_equal(got, want.astype(np.float32))

"""bench.py --gpus N with no outside launcher starts its own N rank processes
(VERDICT r02 "Next round" #1).  On CPU the rank body is tests/spawn_rank_stub.py,
with the oracle standing in for each rank's GPU: what is under test is the
spawner -- the world it forms, the environment each rank gets, rank 0's single
line on stdout, and that a failing rank fails the run instead of leaving the
others waiting."""
import json
import os
import subprocess
import sys
import time

import pytest

import bench

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STUB = os.path.join(ROOT, "tests", "spawn_rank_stub.py")
FAKE = os.path.join(ROOT, "tests", "bench_fake_rank.py")


def _run_spawner(n, env_extra=None, timeout=120, script=STUB, argv=()):
    """bench.spawn_ranks in a child Python, so its stdout is capturable."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBF_BENCH_BACKEND")}
    env.update(env_extra or {})
    code = (f"import sys; sys.path.insert(0, {ROOT!r}); import bench; "
            f"sys.exit(bench.spawn_ranks({n}, {list(argv)!r}, script={script!r}))")
    return subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=timeout,
                          cwd=ROOT)


@pytest.mark.parametrize("n", [2, 4])
def test_spawner_forms_world_and_rank0_prints_one_line(n):
    p = _run_spawner(n)
    assert p.returncode == 0, p.stderr[-2000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    assert out["n_gpus"] == n
    assert out["per_rank"] == [1] * n
    assert out["first_chunk_per_rank"] == [24 * r for r in range(n)]
    assert out["local_rank"] == list(range(n))
    assert out["slice_hash_ok"] is True
    assert out["master"][0] == "127.0.0.1"
    # no GPU here: fewer devices than ranks -> the spawner picks gloo itself
    assert out["backend"] == "gloo"
    assert out["launcher"] == "bench.py"


def test_spawner_failing_rank_fails_the_run_and_stops_the_others():
    t0 = time.time()
    p = _run_spawner(3, {"STUB_FAIL_RANK": "1"}, timeout=90)
    assert p.returncode == 3, (p.returncode, p.stderr[-2000:])
    assert "rank 1 exited with 3" in p.stderr
    assert p.stdout.strip() == ""
    assert time.time() - t0 < 60


def test_rank_env_matches_torchrun_contract():
    envs = bench.rank_env({"X": "1"}, 3, 29555, backend="gloo")
    assert [e["RANK"] for e in envs] == ["0", "1", "2"]
    assert [e["LOCAL_RANK"] for e in envs] == ["0", "1", "2"]
    for e in envs:
        assert e["WORLD_SIZE"] == "3" and e["LOCAL_WORLD_SIZE"] == "3"
        assert e["MASTER_ADDR"] == "127.0.0.1" and e["MASTER_PORT"] == "29555"
        assert e["LBF_BENCH_BACKEND"] == "gloo" and e["X"] == "1"
    assert "LBF_BENCH_BACKEND" not in bench.rank_env({}, 2, 1)[0]


def test_world_mismatch_under_outside_launcher_is_refused(monkeypatch):
    """Under torch.distributed.run with WORLD_SIZE != --gpus the bench refuses to
    run instead of measuring a different world."""
    monkeypatch.setenv("WORLD_SIZE", "1")
    monkeypatch.setenv("RANK", "0")

    class A:
        gpus = 8
    with pytest.raises(SystemExit, match="WORLD_SIZE is 1"):
        bench.dist_setup(A())


_GLOO_CHILD = r'''
import os, sys
sys.path.insert(0, {root!r})
import bench
import torch.distributed as dist
os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=sys.argv[2])
with bench._stdout_to_stderr():
    dist.init_process_group("gloo", rank=int(sys.argv[1]), world_size=2)
dist.barrier()
print('{{"rank": %s}}' % sys.argv[1], flush=True)
dist.destroy_process_group()
'''


def test_gloo_connect_notice_stays_off_stdout(tmp_path):
    """gloo's C++ side prints "[Gloo] Rank r is connected ..." on stdout while the
    group forms; under torch.distributed.run that would land next to rank 0's
    JSON line.  dist_setup forms the group with stdout pointed at stderr."""
    script = tmp_path / "child.py"
    script.write_text(_GLOO_CHILD.format(root=ROOT))
    port = str(bench._free_port())
    procs = [subprocess.Popen([sys.executable, str(script), str(r), port], stdout=subprocess.PIPE,
                              stderr=subprocess.PIPE, text=True) for r in range(2)]
    outs = [p.communicate(timeout=120) for p in procs]
    assert all(p.returncode == 0 for p in procs), [e[-2000:] for _, e in outs]
    for r, (out, err) in enumerate(outs):
        assert out.strip() == '{"rank": %d}' % r, out
        assert "[Gloo]" in err


# What an N>1 line must carry for the driver's 1/2/4/8-GPU record (VERDICT r03
# "Next round" #1): the device-resident value with its roofline, the CPU
# comparator timed in the same run, per-rank golden parity, and both
# host-memory legs.
N_LINE_KEYS = {"metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling",
               "vs_baseline", "dtype", "data", "config", "roofline", "compute_floor", "cpu_baseline", "parity",
               "ranks", "e2e", "e2e_inprocess", "digest_check", "first_chunk_b64"}
PLAIN_ARGV = ["--steps", "2", "--warmup", "1", "--file-gib", "0.0625"]
# everything beyond the timed steps (parity, host-memory legs, cpu_baseline) is behind --full
FAKE_ARGV = PLAIN_ARGV + ["--full", "--cpu-min-s", "0.3"]


def _check_line(out, n):
    assert N_LINE_KEYS <= set(out), N_LINE_KEYS - set(out)
    assert out["n_gpus"] == n and out["scaling"] == "weak" and out["value"] > 0
    r = out["roofline"]
    assert r["bound"] == "hbm" and r["unit"] == "GB/s" and r["peak"] == 8000.0 and r["achieved"] > 0
    assert r["aggregate_peak"] == n * 8000.0 and abs(r["aggregate_achieved"] - n * r["achieved"]) <= 0.01 * n
    cb = out["cpu_baseline"]
    assert cb["kind"] == "port" and cb["unit"] == "GiB/s" and cb["value"] > 0 and cb["cores"] >= 1
    assert cb["parity_vs_gpu"] is True and cb["host"]["usable_cores"] >= 1
    assert "rank 0 alone" in cb["when"]
    assert out["parity"]["per_rank"] == [-1] * n  # no golden at this size
    assert out["e2e"]["parity"] is True and out["e2e"]["parity_per_rank"] == [1] * n
    # the default route (staging), the opt-in on-the-fly route with its first pass, the caller's registration
    for leg in ("pageable", "autopin", "registered"):
        assert len(out["e2e"][leg]["per_rank_gibs"]) == n and out["e2e"][leg]["aggregate_gibs"] > 0, leg
    assert len(out["e2e"]["autopin"]["first_pass_per_rank_gibs"]) == n
    assert "error" not in out["e2e_inprocess"], out["e2e_inprocess"]
    assert out["e2e_inprocess"]["parity"] is True and out["e2e_inprocess"]["parity_per_slice"] == [1] * n
    assert 0 <= out["e2e_inprocess"]["pageable_direct_fraction"] <= 1


@pytest.mark.parametrize("n", [2, 8])
def test_n_rank_line_carries_cpu_baseline_and_every_leg(n):
    """bench.py's own main() in every rank (device calls on host stand-ins,
    tests/bench_fake_rank.py), self-launched as the driver does at N GPUs."""
    p = _run_spawner(n, script=FAKE, argv=["--gpus", str(n)] + FAKE_ARGV, timeout=300)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    _check_line(out, n)
    assert out["ranks"]["process_group"] == "gloo" and out["ranks"]["launcher"] == "bench.py"
    assert "other_configs" not in out


def test_one_rank_group_takes_the_n_rank_route():
    """LBF_BENCH_FORM_GROUP=1 at --gpus 1 forms a one-rank group and runs the
    N>1 flow (its -m gpu twin uses RCCL: tests/test_gpu_nccl.py)."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench._free_port()),
               LBF_BENCH_FORM_GROUP="1", LBF_BENCH_BACKEND="gloo")
    p = subprocess.run([sys.executable, FAKE, "--gpus", "1"] + FAKE_ARGV, env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([x for x in p.stdout.splitlines() if x.strip()][-1])
    _check_line(out, 1)
    assert out["ranks"]["process_group"] == "gloo"


def test_self_launch_refused_under_a_profiler():
    """under rocprofv3 a self-launching bench.py would start GPU
    children from a process the profiler's preload has initialised."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    # rocprofv3's tool library as the preload names it (a path that does not
    # exist here: the loader warns and goes on, and bench.py reads the variable)
    env["LD_PRELOAD"] = (env.get("LD_PRELOAD", "") + " /nonexistent/librocprofiler-sdk-tool.so").strip()
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], env=env, capture_output=True,
                       text=True, timeout=120, cwd=ROOT)
    assert p.returncode != 0 and "not allowed under rocprofv3" in p.stderr, (p.returncode, p.stderr[-2000:])


def test_outside_launcher_with_more_ranks_than_gpus_uses_gloo():
    """Under torch.distributed.run the bench picks the process group by the
    self-launch's rule: RCCL refuses two ranks on one device, so with more
    ranks than visible GPUs (here none) and no LBF_BENCH_BACKEND it forms a gloo
    group instead of failing in init_process_group."""
    env = {k: v for k, v in os.environ.items()
           if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBF_BENCH_BACKEND")}
    port = str(bench._free_port())
    p = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2",
                        "--master-addr", "127.0.0.1", "--master-port", port, FAKE, "--gpus", "2"] + FAKE_ARGV,
                       env=env, capture_output=True, text=True, timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([x for x in p.stdout.splitlines() if x.strip().startswith("{")][-1])
    _check_line(out, 2)
    assert out["ranks"]["process_group"] == "gloo"
    assert "process group gloo (rehearsal)" in p.stderr


def test_failing_cpu_baseline_still_prints_the_line():
    """A host-side failure of the CPU comparator (on a node whose host differs
    from the box's) is recorded in cpu_baseline.error; rank 0 still prints the
    line with its device-resident value."""
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK")}
    env.update(RANK="0", LOCAL_RANK="0", WORLD_SIZE="1", MASTER_ADDR="127.0.0.1", MASTER_PORT=str(bench._free_port()),
               LBF_BENCH_FORM_GROUP="1", LBF_BENCH_BACKEND="gloo", FAKE_CPU_BASELINE_FAILS="1")
    p = subprocess.run([sys.executable, FAKE, "--gpus", "1"] + FAKE_ARGV, env=env, capture_output=True, text=True,
                       timeout=300, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    out = json.loads([x for x in p.stdout.splitlines() if x.strip()][-1])
    assert out["value"] > 0 and out["roofline"]["achieved"] > 0
    assert out["cpu_baseline"]["value"] is None and "injected" in out["cpu_baseline"]["error"]


# What only a --full run measures or checks: absent from a plain line.
FULL_ONLY_KEYS = {"cpu_baseline", "e2e", "e2e_inprocess", "e2e_host_to_host_gibs", "e2e_registered", "e2e_autopin",
                  "other_configs", "parity", "digest_check", "first_chunk_b64"}


def _plain_run(extra, timeout=300):
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "LBF_BENCH_FORM_GROUP")}
    p = subprocess.run([sys.executable, FAKE, "--gpus", "1"] + PLAIN_ARGV + list(extra), env=env, capture_output=True,
                       text=True, timeout=timeout, cwd=ROOT)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    return json.loads(lines[0])


def test_plain_run_times_the_steps_and_nothing_else(tmp_path, oracle):
    """Without --full the line holds the headline figure of the --steps timed
    launches and none of the legs that follow them; --dump-outputs writes the
    last launch's digests as float32, the same bytes in every run."""
    import hashlib

    import numpy as np
    outs = [_plain_run(["--dump-outputs", str(tmp_path / d)]) for d in ("a", "b")]
    out = outs[0]
    assert {"metric", "value", "unit", "higher_is_better", "dtype", "ms_per_step", "roofline", "config"} <= set(out)
    assert not FULL_ONLY_KEYS & set(out), FULL_ONLY_KEYS & set(out)
    assert out["steps"] == 2 and out["warmup"] == 1 and out["full"] is False
    assert out["unit"] == "GiB/s" and out["higher_is_better"] is True and out["dtype"] == "u32"
    assert out["value"] > 0 and out["ms_per_step"] > 0 and out["roofline"]["traffic"] is None
    # value is the bytes of the timed steps over their wall time, ms_per_step that time per step
    assert abs(out["value"] * out["ms_per_step"] / 1e3 - 0.0625) < 1e-3 * 0.0625 + 1e-4
    a, b = (np.load(tmp_path / d / "digests.npy") for d in ("a", "b"))
    cs, n = 262144, 256
    assert a.dtype == np.float32 and a.shape == (n, 20) and np.array_equal(a, b)
    data = oracle.synth(0x5EED, 0, n * cs)
    want = np.array([list(hashlib.sha1(data[i * cs:(i + 1) * cs].tobytes()).digest()) for i in range(n)])
    assert np.array_equal(a, want.astype(np.float32))
    assert sorted(os.listdir(tmp_path / "a")) == ["digests.npy"]


def test_dump_outputs_samples_a_large_output(tmp_path):
    """Above the size limit each rank keeps a fixed, seeded sample of its rows:
    the same rows every time, in ascending order, and the files stay below the
    limit together."""
    import numpy as np
    d = (np.arange(5000 * 20) % 251).astype(np.uint8).reshape(5000, 20)
    limit = 64 << 10
    for sub in ("a", "b"):
        for rank in range(2):
            bench.dump_outputs(str(tmp_path / sub), d, rank, 2, max_bytes=limit)
    files = sorted(os.listdir(tmp_path / "a"))
    assert files == ["digests_rank0.npy", "digests_rank0_rows.npy", "digests_rank1.npy", "digests_rank1_rows.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in files) <= limit
    rows = np.load(tmp_path / "a" / "digests_rank0_rows.npy")
    got = np.load(tmp_path / "a" / "digests_rank0.npy")
    assert got.dtype == np.float32 and rows.dtype == np.float64 and len(rows) > 300
    assert np.all(np.diff(rows) > 0) and np.array_equal(got, d[rows.astype(np.int64)].astype(np.float32))
    for f in files:
        assert np.array_equal(np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)), f
    # an output that fits is written whole, with no row file
    bench.dump_outputs(str(tmp_path / "c"), d[:100], 0, 1, max_bytes=limit)
    assert os.listdir(tmp_path / "c") == ["digests.npy"] and np.load(tmp_path / "c" / "digests.npy").shape == (100, 20)

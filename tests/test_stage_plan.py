"""The staging planner (bitflood_amd/csrc/stage_plan.hpp) on the CPU: source
order, job sizing, group packing, piece cutting, the header rule, the cover
test and the wire calls' slot runs, by tests/c/stage_plan_tests.cpp (built by
tests/c/Makefile with plain g++; it links nothing of the library)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CDIR = os.path.join(ROOT, "tests", "c")


def test_stage_plan_program():
    exe = os.path.join(CDIR, "build", "stage_plan_tests")
    subprocess.check_call(["make", "-s", "-C", CDIR, "build/stage_plan_tests"])  # rebuilt when the planner changed
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    assert r.stdout.splitlines()[-1] == "stage_plan_tests: OK", r.stdout

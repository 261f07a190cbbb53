"""Resumable SHA-1 states, the parts that need no GPU: the exported symbols and
the 96-byte record, the pure-Python model that checks forged states
(tests/sha1_model.py), the batch call's planner
(bitflood_amd/csrc/update_plan.hpp, by tests/c/update_plan_tests.cpp, plain
and under ASan/UBSan as stand-alone programs), and the update kernel's
resource usage on gfx950 (no scratch, no spills)."""
import hashlib
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import sha1_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def test_update_symbols_exported():
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in ("lbf_sha1_state_init", "lbf_sha1_update_launch", "lbf_sha1_update_batch"):
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s


def test_state_record_layout_and_init():
    from bitflood_amd import STATE_DTYPE, new_states
    from bitflood_amd import hashing
    assert STATE_DTYPE.itemsize == 96
    assert [STATE_DTYPE.fields[k][1] for k in ("h", "buffered", "total", "block")] == [0, 20, 24, 32]
    assert {"STATE_DTYPE", "new_states", "update_launch"} <= set(hashing.__all__)
    st = new_states(3)
    assert st.shape == (3,) and st.dtype == STATE_DTYPE
    for k in range(3):
        assert st["h"][k].tolist() == [0x67452301, 0xEFCDAB89, 0x98BADCFE, 0x10325476, 0xC3D2E1F0]
    assert not st["buffered"].any() and not st["total"].any() and not st["block"].any()
    # init overwrites whatever was there, all 96 bytes of each record
    st.view(np.uint8)[:] = 0xAB
    _capi.load().lbf_sha1_state_init(st.ctypes.data, 2)
    assert st[:2].tobytes() == new_states(2).tobytes()
    assert st[2:].tobytes() == b"\xAB" * 96
    assert new_states(0).size == 0


def test_model_matches_hashlib_and_oracle(oracle):
    rng = np.random.default_rng(61)
    for size in [0, 1, 55, 56, 63, 64, 65, 119, 120, 127, 128, 129, 1000, 4097]:
        data = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        for _ in range(4):
            cuts = sorted(rng.integers(0, size + 1, int(rng.integers(0, 6))).tolist())
            st = sha1_model.init()
            pos = 0
            for c in cuts + [size]:
                st = sha1_model.update(st, data[pos:c])
                assert st[1] == c and len(st[2]) == c % 64
                pos = c
            got = sha1_model.final(st)
            assert got == hashlib.sha1(data).digest()
            assert got == oracle.sha1_incremental(data, cuts)


def _build_plan_tests(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra,
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                         os.path.join(ROOT, "tests", "c", "update_plan_tests.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,extra", [("plain", []),
                                        ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])])
def test_update_plan_program(tmp_path, name, extra):
    """Refusals, cutting and run packing of update_plan.hpp, as a stand-alone
    program (no preload, no Python under a sanitizer)."""
    exe = _build_plan_tests(tmp_path, "update_plan_tests_" + name, extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "update_plan_tests: OK", r.stdout


def test_update_plan_header_is_hip_free():
    text = open(os.path.join(CSRC, "update_plan.hpp")).read()
    assert "hip/" not in text and "lbf_internal.hpp" not in text and "lbf_host.hpp" not in text


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_update_kernel_has_no_scratch_and_no_spills(tmp_path):
    """A register array indexed by the state's `buffered` would go to scratch;
    the kernel tops the block up in the record in memory instead."""
    src = os.path.join(CSRC, "sha1_update.hip")
    assert "sha1_update.hip" in subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True,
                                               text=True, check=True).stdout.split()
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / "u.o"),
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks}
    upd = [b for name, b in kernels.items() if "sha1_update_kernel" in name]
    assert len(upd) == 1, sorted(kernels)
    rem = upd[0]
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
    assert re.search(r"Dynamic Stack: False", rem), rem

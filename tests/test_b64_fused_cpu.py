"""The fused route of the piecewise base64 decode (bitflood_amd/csrc/
b64_update_fused.hip), the parts that need no GPU: the switch and its
environment variable, the source list, and the kernel's resource usage on
gfx950 beside the three stage kernels it is built from."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from bitflood_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_symbol_and_switch():
    import bitflood_amd
    from bitflood_amd import hashing
    lib = _capi.load()
    assert "lbf_set_b64_fused" in _capi.header_symbols() and "lbf_set_b64_fused" in _capi._SIGS
    assert hasattr(lib, "lbf_set_b64_fused")
    assert "set_b64_fused" in hashing.__all__ and bitflood_amd.set_b64_fused is hashing.set_b64_fused
    # the switch needs no GPU: it returns the previous value
    first = hashing.set_b64_fused(True)
    assert hashing.set_b64_fused(False) is True
    assert hashing.set_b64_fused(first) is False
    assert lib.lbf_abi_version() == 1  # a switch beside the other two: the ABI's version stays
    header = re.sub(r"\s*\n \* ", " ", open(_capi.HEADER_PATH).read())
    assert "three enqueues whatever the other two switches say" in header
    assert "are the same on both routes" in header


@pytest.mark.parametrize("env,want", [(None, 0), ("0", 0), ("1", 1), ("", 0), ("11", 0)])
def test_initial_value_comes_from_the_environment(env, want):
    """A fresh process: off unless LBF_B64_FUSED is exactly "1"; the first call
    reports the initial value."""
    environ = {k: v for k, v in os.environ.items() if k != "LBF_B64_FUSED"}
    if env is not None:
        environ["LBF_B64_FUSED"] = env
    code = ("from bitflood_amd import _capi; lib = _capi.load(); "
            "print(lib.lbf_set_b64_fused(0), lib.lbf_set_b64_fused(1))")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT, env=environ,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert r.stdout.split() == [str(want), "0"], r.stdout


def test_fused_kernel_is_in_the_source_list():
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert "b64_update_fused.hip" in srcs
    assert {"b64_update.hip", "b64_update_lines.hip", "b64_flat.hip"} <= set(srcs)


def _resources(name, tmp_path):
    """{kernel name: its remarks} of one translation unit, cross-compiled for gfx950."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / (name + ".o")),
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, name)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    return {b.split()[0]: b for b in blocks}


def _number(rem, what):
    return int(re.search(re.escape(what) + r": (\d+)", rem).group(1))


@needs_hipcc
def test_fused_kernel_resources(tmp_path):
    """One kernel: nothing in scratch, no vector register spilled, an occupancy
    no lower than the lowest of the three stage kernels built from the same
    tree, and one LDS allocation shared by the stages (two staged tiles of text
    or the scan's sextets, never both)."""
    fused = _resources("b64_update_fused.hip", tmp_path)
    assert len(fused) == 1 and "b64_update_fused_kernel" in next(iter(fused)), sorted(fused)
    rem = next(iter(fused.values()))
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"Dynamic Stack: False", rem), rem
    stages = {}
    for unit, kernel in (("b64_update_lines.hip", "b64_update_lines_kernel"),
                         ("b64_flat.hip", "b64_update_flat_kernel"), ("b64_update.hip", "b64_update_kernel")):
        found = [v for k, v in _resources(unit, tmp_path).items() if kernel in k]
        assert len(found) == 1, (unit, kernel)
        stages[kernel] = found[0]
    occupancy = {k: _number(v, "Occupancy [waves/SIMD]") for k, v in stages.items()}
    assert _number(rem, "Occupancy [waves/SIMD]") >= min(occupancy.values()), (rem, occupancy)
    assert _number(rem, " VGPRs") <= 64, rem  # eight waves a SIMD
    lds = _number(rem, "LDS Size [bytes/block]")
    tiles = max(_number(stages[k], "LDS Size [bytes/block]")
                for k in ("b64_update_lines_kernel", "b64_update_flat_kernel"))
    scan = _number(stages["b64_update_kernel"], "LDS Size [bytes/block]")
    assert 2 * 5256 <= lds <= tiles + 64 < tiles + scan - 4096, (lds, tiles, scan)
    text = "".join(open(os.path.join(CSRC, name)).read()
                   for name in ("b64_update_fused.hip", "b64_update_stages.hpp", "b64_device.hpp"))
    assert "asm" not in text.replace("__launch_bounds__", "")  # no inline assembly: only barriers synchronise
    assert "while (" not in text and "__syncthreads()" in text
    # atomics go to LDS only (the scan's first '='), and every stage is stated once, in the header
    assert re.findall(r"\batomic[A-Z]\w*\([^)]*\)", text) == ["atomicMin(first_eq, pos)"]
    for unit in ("b64_update_lines.hip", "b64_flat.hip", "b64_update.hip", "b64_update_fused.hip"):
        assert '#include "b64_update_stages.hpp"' in open(os.path.join(CSRC, unit)).read(), unit

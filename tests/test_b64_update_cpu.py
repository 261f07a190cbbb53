"""The resumable base64 decode, the parts that need no GPU: the piecewise
model (tests/wire_piece_model.py) against xmlrpc++'s recorded answers at every
cutting, the exported symbols and the 16-byte record, the batch call's planner
(bitflood_amd/csrc/b64_update_plan.hpp, by tests/c/b64_update_plan_tests.cpp,
plain and under ASan/UBSan as stand-alone programs), and the decode kernel's
resource usage on gfx950 (no scratch, no spills)."""
import itertools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_layouts as W
from tests import wire_piece_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def tiny_texts():
    """All 5,461 texts of length <= 6 over a sextet, another, '=' and junk."""
    return [bytes(t) for n in range(7) for t in itertools.product(b"AQ=*", repeat=n)]


def test_model_gives_what_xmlrpc_recorded_at_every_cut(golden):
    rows = golden("xmlrpc07_base64_get.json")["get"]
    assert len(rows) == 363
    cuttings = 0
    for text, want in ((bytes.fromhex(r[0]), bytes.fromhex(r[1])) for r in rows):
        n = len(text)
        for a in range(n + 1):
            assert M.decode_pieces([text[:a], text[a:]]) == want, (text, a)
            assert M.decode_pieces([text[:a], text[a:]], M.update_by_character) == want, (text, a)
            cuttings += 1
            if n <= 14:
                for b in range(a, n + 1):
                    assert M.decode_pieces([text[:a], text[a:b], text[b:]]) == want, (text, a, b)
                    assert M.decode_pieces([text[:a], text[a:b], text[b:]], M.update_by_character) == want
                    cuttings += 1
    assert cuttings == 18129


def test_model_on_every_tiny_text_at_every_cut():
    texts = tiny_texts()
    assert len(texts) == 5461
    for t in texts:
        want = W.b64get(t)
        assert W.decode(t) == want
        for a in range(len(t) + 1):
            st, first = M.update(M.init(), t[:a])
            assert (st, first) == M.update_by_character(M.init(), t[:a])
            assert M.update(st, t[a:]) == M.update_by_character(st, t[a:])
            decoded, carry, ended = st
            assert first == want[:len(first)] and decoded == len(first) and len(carry) <= 3
            assert ended or decoded % 3 == 0
            st, rest = M.update(st, t[a:])
            assert first + rest == want and M.final(st) == len(want), (t, a)


def test_symbols_exported_and_record_layout():
    from bitflood_amd import B64_STATE_DTYPE, hashing, new_b64_states
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in ("lbf_b64_state_init", "lbf_b64_update_launch", "lbf_b64_update_batch"):
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s
    assert {"B64_STATE_DTYPE", "new_b64_states", "b64_update_launch"} <= set(hashing.__all__)
    assert hasattr(hashing.ChunkHasher, "update_text")
    assert B64_STATE_DTYPE.itemsize == 16
    assert [B64_STATE_DTYPE.fields[k][1] for k in ("decoded", "carry", "ncarry", "ended", "zero")] == [0, 8, 12, 13, 14]
    header = open(_capi.HEADER_PATH).read()
    rec = header[header.index("typedef struct lbf_b64_state {"):header.index("} lbf_b64_state;")]
    assert re.findall(r"(uint\d+_t)\s+(\w+);", rec) == [("uint64_t", "decoded"), ("uint32_t", "carry"),
                                                        ("uint8_t", "ncarry"), ("uint8_t", "ended"),
                                                        ("uint16_t", "zero")]
    # init needs no GPU and overwrites all 16 bytes of each record it is given
    st = new_b64_states(3)
    assert st.shape == (3,) and st.tobytes() == bytes(48)
    st.view(np.uint8)[:] = 0xAB
    lib.lbf_b64_state_init(st.ctypes.data, 2)
    assert st.tobytes() == bytes(32) + b"\xAB" * 16
    assert new_b64_states(0).size == 0
    assert M.b64_records([M.init()], B64_STATE_DTYPE).tobytes() == new_b64_states(1).tobytes()


def _build_plan_tests(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra,
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                         os.path.join(ROOT, "tests", "c", "b64_update_plan_tests.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,extra", [("plain", []),
                                        ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])])
def test_b64_update_plan_program(tmp_path, name, extra):
    """Refusals, the decode bound, device places and copy-back runs of
    b64_update_plan.hpp, as a stand-alone program (no preload, no Python under a
    sanitizer)."""
    exe = _build_plan_tests(tmp_path, "b64_update_plan_tests_" + name, extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "b64_update_plan_tests: OK", r.stdout


def test_b64_update_plan_header_is_hip_free():
    for name in ("b64_update_plan.hpp", "update_plan.hpp", "stage_plan.hpp"):  # it and what it includes
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "lbf_internal.hpp" not in text and "lbf_host.hpp" not in text, name


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_b64_update_kernel_has_no_scratch_and_no_spills(tmp_path):
    """The lane's sixteen characters and twelve bytes stay in registers, and
    the sextets go through LDS: 4,096 + 16 of them, the table and the scan sums."""
    src = os.path.join(CSRC, "b64_update.hip")
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert "b64_update.hip" in srcs and "update_batch.cpp" in srcs
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / "u.o"),
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks}
    assert len(kernels) == 2, sorted(kernels)
    for name, rem in kernels.items():
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
        assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
        assert re.search(r"Dynamic Stack: False", rem), rem
    dec = [rem for name, rem in kernels.items() if "b64_update_kernel" in name]
    assert len(dec) == 1, sorted(kernels)
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", dec[0]).group(1))
    assert 4096 + 3 + 256 + 16 <= lds <= 5120, lds  # occupancy is not LDS-bound
    text = open(src).read()
    assert "asm" not in text.replace("__launch_bounds__", "")  # no inline assembly, and only barriers synchronise
    assert "while (" not in text

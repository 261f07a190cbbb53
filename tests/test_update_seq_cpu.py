"""Several pieces of one chain per call, the parts that need no GPU: the
exported symbols and bindings, chain_table, the batch calls' planner
(bitflood_amd/csrc/update_plan.hpp and b64_update_plan.hpp, by tests/c/update_seq_plan_tests.cpp,
plain and under ASan/UBSan as stand-alone programs), and the two new kernels'
resource usage on gfx950 (no scratch, no spills, no dynamic stack)."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SYMBOLS = ("lbf_sha1_update_seq_launch", "lbf_sha1_update_seq_batch", "lbf_b64_update_seq_launch",
           "lbf_b64_update_seq_batch")


def test_seq_symbols_exported():
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in SYMBOLS:
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s
    # the calls that take one piece per state have the same arguments, but for the chain table
    sigs = _capi._SIGS
    assert sigs["lbf_sha1_update_seq_batch"] == sigs["lbf_sha1_update_batch"]
    assert sigs["lbf_b64_update_seq_batch"] == sigs["lbf_b64_update_batch"]
    assert len(sigs["lbf_sha1_update_seq_launch"][1]) == len(sigs["lbf_sha1_update_launch"][1]) + 2
    assert len(sigs["lbf_b64_update_seq_launch"][1]) == len(sigs["lbf_b64_update_launch"][1]) + 2


def test_seq_bindings_exported():
    import bitflood_amd
    from bitflood_amd import ChunkHasher, hashing
    names = {"chain_table", "update_seq_launch", "b64_update_seq_launch"}
    assert names <= set(hashing.__all__)
    for n in names:
        assert getattr(bitflood_amd, n) is getattr(hashing, n)
    assert callable(ChunkHasher.update_chunks_seq) and callable(ChunkHasher.update_text_seq)


def _check_table(state_of):
    from bitflood_amd import chain_table
    state_of = np.asarray(state_of, dtype=np.uint32)
    order, chain_state, chain_first = chain_table(state_of)
    assert order.dtype == chain_state.dtype == chain_first.dtype == np.uint32
    n = state_of.size
    assert sorted(order.tolist()) == list(range(n))  # a permutation
    assert chain_first.size == chain_state.size + 1 and chain_first[0] == 0 and chain_first[-1] == n
    assert len(set(chain_state.tolist())) == chain_state.size  # one chain per state
    firsts = []
    for c, s in enumerate(chain_state):
        pieces = order[chain_first[c]:chain_first[c + 1]].tolist()
        assert pieces and pieces == sorted(pieces)  # a chain's pieces keep their order
        assert pieces == np.flatnonzero(state_of == s).tolist()  # and are all of the state's
        firsts.append(pieces[0])
    assert firsts == sorted(firsts)  # chains stand in the order of their first pieces
    # round trip: the state of every piece, from the table
    back = np.empty(n, dtype=np.uint32)
    back[order] = np.repeat(chain_state, np.diff(chain_first.astype(np.int64)))
    assert np.array_equal(back, state_of)
    return order, chain_state, chain_first


def test_chain_table_round_trips():
    order, chain_state, chain_first = _check_table([5, 2, 5, 7, 2, 5])
    assert order.tolist() == [0, 2, 5, 1, 4, 3]
    assert chain_state.tolist() == [5, 2, 7] and chain_first.tolist() == [0, 3, 5, 6]
    # no state repeats: the identity, whatever the order of the states
    order, chain_state, chain_first = _check_table([9, 3, 4, 0])
    assert order.tolist() == [0, 1, 2, 3] and chain_state.tolist() == [9, 3, 4, 0]
    assert chain_first.tolist() == [0, 1, 2, 3, 4]
    _check_table([4, 4, 4])
    _check_table([0xFFFFFFFF, 0, 0xFFFFFFFF])
    order, chain_state, chain_first = _check_table([])
    assert order.size == 0 and chain_state.size == 0 and chain_first.tolist() == [0]
    rng = np.random.default_rng(12)
    for n, states in ((1, 1), (50, 7), (300, 300), (1000, 40)):
        _check_table(rng.integers(0, states, n))


def _build_plan_tests(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra,
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                         os.path.join(ROOT, "tests", "c", "update_seq_plan_tests.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,extra", [("plain", []),
                                        ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-omit-frame-pointer"])])
def test_update_seq_plan_program(tmp_path, name, extra):
    """Grouping, straddling chains, every refusal, text areas and copy-back
    ranges of the seq calls' planner, as a stand-alone program (no preload, no
    Python under a sanitizer)."""
    exe = _build_plan_tests(tmp_path, "update_seq_plan_tests_" + name, extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "update_seq_plan_tests: OK", r.stdout


def test_update_seq_plan_header_is_hip_free():
    for name in ("update_plan.hpp", "b64_update_plan.hpp", "stage_plan.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip/" not in text and "lbf_internal.hpp" not in text and "lbf_host.hpp" not in text, name


def _kernel_remarks(unit, kernel, tmp_path):
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert unit in srcs, srcs
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / (unit + ".o")),
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, unit)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    found = [b for b in blocks if kernel in b.split()[0]]
    assert len(found) == 1, [b.split()[0] for b in blocks]
    return found[0]


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
@pytest.mark.parametrize("unit,kernel", [("sha1_update_seq.hip", "sha1_update_seq_kernel"),
                                         ("b64_update_seq.hip", "b64_update_seq_kernel")])
def test_seq_kernels_have_no_scratch_and_no_spills(tmp_path, unit, kernel):
    """The hash kernel holds the record's header in registers over the chain's
    pieces and the decode kernel the decoder's record; neither may pay for the
    loop with scratch, spilled registers (scalar ones parked in vector lanes
    included) or a dynamic stack.  No occupancy is forced."""
    rem = _kernel_remarks(unit, kernel, tmp_path)
    print(rem)
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
    assert re.search(r"Dynamic Stack: False", rem), rem
    text = open(os.path.join(CSRC, unit)).read()
    assert "amdgpu_waves_per_eu" not in text and "amdgpu_flat_work_group_size" not in text


def test_decode_kernel_is_built_from_the_shared_stages():
    text = open(os.path.join(CSRC, "b64_update_seq.hip")).read()
    assert '#include "b64_update_stages.hpp"' in text
    for fn in ("read_rec(", "lines_stage(", "flat_stage(", "scan_stage(", "rec_words("):
        assert fn in text, fn
    assert "b64_fused_enabled" not in text  # the route does not depend on lbf_set_b64_fused

"""lbf_b64_verify_launch, the parts that need no GPU: the two symbols and
their bindings, every refusal the launch makes before it enqueues anything,
the kernel set of the new translation unit and its kernels' resource usage on
gfx950, and where the kernels' bodies come from."""
import inspect
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest

from bitflood_amd import _capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
UNIT = "b64_verify_launch.hip"
KERNELS = ("b64_decode_routed_kernel", "b64_decode_scan_kernel", "b64_verify_finish_kernel")
WHO = b"lbf_b64_verify_launch"
GIB = 1 << 30
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _refused(lib, rc, *words):
    msg = lib.lbf_last_error() or b""
    assert rc == _capi.LBF_ERR_INVALID, (rc, msg)
    for w in (WHO,) + words:
        assert w in msg, (w, msg)


def test_both_symbols_are_exported_and_bound(lib):
    for name in ("lbf_b64_verify_launch", "lbf_b64_verify_launch_work"):
        assert name in _capi._SIGS and name in _capi.header_symbols()
        assert getattr(lib, name).argtypes == _capi._SIGS[name][1]
    assert len(_capi._SIGS["lbf_b64_verify_launch"][1]) == 15
    assert lib.lbf_abi_version() == 1
    text = open(_capi.HEADER_PATH).read()
    assert re.search(r"#define LBF_ABI_VERSION 1\b", text)
    assert len(re.findall(r"\bint lbf_b64_verify_launch\(", text)) == 1


def test_python_helpers():
    import bitflood_amd
    from bitflood_amd import hashing
    for name in ("verify_b64_launch", "b64_verify_launch_work"):
        assert name in hashing.__all__ and getattr(bitflood_amd, name) is getattr(hashing, name)
    p = inspect.signature(hashing.verify_b64_launch).parameters
    assert list(p) == ["text", "text_offsets", "text_lens", "n", "max_text_len", "expected_sizes", "max_size", "out",
                       "out_offsets", "out_sizes", "work", "digests", "expected", "verdicts", "stream"]
    assert all(p[k].default is None for k in ("digests", "expected", "verdicts", "stream"))


@pytest.mark.parametrize("n", [0, 1, 7, 65537, (1 << 31) - 1, 1 << 40])
def test_work_is_two_bytes_a_chunk(lib, n):
    from bitflood_amd import b64_verify_launch_work
    assert lib.lbf_b64_verify_launch_work(n) == 2 * n == b64_verify_launch_work(n)


def _tables(n=1):
    """Host arrays standing in for every table of the call (the refusals below
    come before any of them is read)."""
    return dict(text=np.zeros(512, np.uint8), toff=np.zeros(n, np.uint64), tlen=np.full(n, 136, np.uint32),
                cap=np.full(n, 100, np.uint32), out=np.zeros(512, np.uint8), ooff=np.zeros(n, np.uint64),
                osz=np.zeros(n, np.uint32), dig=np.zeros(20 * n + 4, np.uint8), exp=np.zeros(20 * n + 4, np.uint8),
                ver=np.zeros(n, np.uint8), work=np.zeros(2 * n, np.uint8))


def _launch(lib, t, n=1, max_text_len=136, max_size=100, null=(), shift=None):
    p = {k: (None if k in null else v.ctypes.data + (shift or {}).get(k, 0)) for k, v in t.items()}
    return lib.lbf_b64_verify_launch(p["text"], p["toff"], p["tlen"], n, max_text_len, p["cap"], max_size, p["out"],
                                     p["ooff"], p["osz"], p["dig"], p["exp"], p["ver"], p["work"], None)


@pytest.mark.parametrize("table", ["text", "toff", "tlen", "cap", "out", "ooff", "osz", "work"])
def test_refuses_a_null_required_argument(lib, table):
    _refused(lib, _launch(lib, _tables(), null=(table,)), b"null")


def test_refuses_too_many_chunks(lib):
    _refused(lib, _launch(lib, _tables(), n=1 << 31), b"2^31-1")


def test_refuses_bounds_over_the_wire_decodes(lib):
    _refused(lib, _launch(lib, _tables(), max_size=GIB + 1), b"1 GiB")
    _refused(lib, _launch(lib, _tables(), max_text_len=3 * (GIB // 2) + 1), b"1.5 GiB")
    assert GIB < 3 * (GIB // 2) < 1 << 32


@pytest.mark.parametrize("table,by", [("toff", 4), ("tlen", 2), ("cap", 1), ("ooff", 4), ("osz", 2)])
def test_refuses_a_misaligned_table(lib, table, by):
    t = _tables(n=2)
    _refused(lib, _launch(lib, t, n=1, shift={table: by}), b"not aligned to its element size")


@pytest.mark.parametrize("table", ["dig", "exp"])
def test_refuses_digest_arrays_off_four_bytes(lib, table):
    _refused(lib, _launch(lib, _tables(), shift={table: 2}), b"4-byte aligned")


def test_refuses_expected_without_verdicts_and_the_reverse(lib):
    _refused(lib, _launch(lib, _tables(), null=("ver",)), b"expected and verdicts go together")
    _refused(lib, _launch(lib, _tables(), null=("exp",)), b"expected and verdicts go together")


def test_no_chunks_is_ok_whatever_else_is_passed(lib):
    assert lib.lbf_b64_verify_launch(None, None, None, 0, 0, None, 0, None, None, None, None, None, None, None,
                                     None) == 0
    assert _launch(lib, _tables(), n=0, max_size=GIB + 1, max_text_len=0xFFFFFFFF, null=("ver", "work")) == 0


@needs_hipcc
def test_the_new_source_holds_exactly_the_three_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_digest
    got = isa_digest.digests(os.path.join(CSRC, UNIT))
    assert len(got) == 3, sorted(got)
    for k in KERNELS:
        assert sum(k in name for name in got) == 1, (k, sorted(got))
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert UNIT in srcs


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("verify_launch") / "k.o"
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(out),
                        "-Rpass-analysis=kernel-resource-usage", os.path.join(CSRC, UNIT)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return re.split(r"remark: Function Name: ", r.stderr)[1:]


@needs_hipcc
@pytest.mark.parametrize("kernel", KERNELS)
def test_kernels_have_no_scratch_no_spills_and_no_dynamic_stack(remarks, kernel):
    found = [b for b in remarks if kernel in b.split()[0]]
    assert len(found) == 1, [b.split()[0] for b in remarks]
    rem = found[0]
    print(rem)
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
    assert re.search(r"Dynamic Stack: False", rem), rem


def _kernel_text(text, kernel):
    """The source of one kernel: from its name to the next __global__ (or the end of the kernels' namespace)."""
    a = text.index(kernel + "(")
    rest = text[a:]
    b = [rest.find(m) for m in ("__global__", "}  // namespace")]
    return rest[:min(x for x in b if x > 0)]


def test_kernels_are_built_from_the_shared_stages_and_tile_bodies():
    text = open(os.path.join(CSRC, UNIT)).read()
    for h in ("b64_update_stages.hpp", "b64_decode_tiles.hpp", "b64_flat.hpp"):
        assert '#include "%s"' % h in text, h
    assert "kern_b64.hpp" not in text  # its kernels are compiled once, in sha1_kernels.hip
    scan = _kernel_text(text, "b64_decode_scan_kernel")
    assert "b64s::scan_stage(" in scan and "b64s::Rec r{0, 0u, 0u, false}" in scan
    assert "__device__" not in text  # no stage or body of its own: the kernels call the headers'
    assert "scan_stage(Rec& r, const Piece& pc" in open(os.path.join(CSRC, "b64_update_stages.hpp")).read()
    routed = _kernel_text(text, "b64_decode_routed_kernel")
    assert "b64_flat_candidate(len, cap)" in routed
    assert "b64_flat_decode_tiles(" in routed and "b64_canon_decode_tiles(" in routed
    assert "b64_flat_enabled" not in text  # the route does not depend on lbf_set_b64_flat
    tiles = re.sub(r"//[^\n]*", "", open(os.path.join(CSRC, "b64_decode_tiles.hpp")).read())  # the code alone
    assert "__global__" not in tiles and "__constant__" not in tiles and "__shared__" not in tiles
    # the old kernels are built from the same block, tile and geometry
    assert '#include "b64_decode_tiles.hpp"' in open(os.path.join(CSRC, "kern_b64.hpp")).read()
    assert '#include "b64_decode_tiles.hpp"' in open(os.path.join(CSRC, "b64_flat.hip")).read()


def test_flat_candidate_is_the_hosts_rule(lib):
    """The routed kernel and lbf_b64_verify_batch read one rule (b64_flat.hpp);
    it names lbf_b64_put_length through b64e::text_length."""
    hpp = open(os.path.join(CSRC, "b64_flat.hpp")).read()
    assert "text_len != b64e::text_length(cap, false)" in hpp
    assert "lbf_b64_put_length(uint64_t size) { return b64e::text_length(size, false); }" in \
        open(os.path.join(CSRC, "wire_batch.cpp")).read()

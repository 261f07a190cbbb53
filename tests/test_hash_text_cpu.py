"""lbf_sha1_hashes_launch and lbf_verify_hashes_launch, the parts that need no
GPU: the three symbols and their bindings, the work formula, every refusal the
launches make before they enqueue anything, the kernel set of hash_text.hip and
its kernels' resource usage on gfx950, and where its alphabet comes from."""
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
UNIT = "hash_text.hip"
KERNELS = ("hash_text_encode_kernel", "hash_text_compare_kernel", "hash_text_scan_kernel", "hash_text_scatter_kernel")
SYMBOLS = ("lbf_sha1_hashes_launch", "lbf_verify_hashes_launch", "lbf_verify_hashes_launch_work")
HASHES, VERIFY = b"lbf_sha1_hashes_launch", b"lbf_verify_hashes_launch"
needs_hipcc = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _refused(lib, rc, who, *words):
    msg = lib.lbf_last_error() or b""
    assert rc == _capi.LBF_ERR_INVALID, (rc, msg)
    assert msg.startswith(who + b":"), msg
    for w in words:
        assert w in msg, (w, msg)


def test_the_three_symbols_are_declared_once_exported_and_bound(lib):
    text = open(_capi.HEADER_PATH).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in SYMBOLS:
        assert name in _capi._SIGS and name in _capi.header_symbols()
        assert getattr(lib, name).argtypes == _capi._SIGS[name][1]
        assert len(re.findall(r"\b%s\s*\(" % name, code)) == 1, name
    assert len(_capi._SIGS["lbf_sha1_hashes_launch"][1]) == 9
    assert len(_capi._SIGS["lbf_verify_hashes_launch"][1]) == 13
    assert lib.lbf_abi_version() == 1
    assert re.search(r"#define LBF_ABI_VERSION 1\b", text)


def test_python_helpers():
    import bitflood_amd
    from bitflood_amd import hashing
    for name in ("sha1_hashes_launch", "verify_hashes_launch", "verify_hashes_launch_work"):
        assert name in hashing.__all__ and getattr(bitflood_amd, name) is getattr(hashing, name)
    p = inspect.signature(hashing.sha1_hashes_launch).parameters
    assert list(p) == ["base", "offsets", "sizes", "n", "hashes", "work", "hash_offsets", "digests", "stream"]
    assert all(p[k].default is None for k in ("hash_offsets", "digests", "stream"))
    p = inspect.signature(hashing.verify_hashes_launch).parameters
    assert list(p) == ["base", "offsets", "sizes", "n", "hashes", "chunkmap", "work", "hash_offsets", "hash_lens",
                       "missing", "missing_count", "digests", "stream"]
    assert all(p[k].default is None for k in ("hash_offsets", "hash_lens", "missing", "missing_count", "digests",
                                              "stream"))
    assert list(inspect.signature(hashing.verify_hashes_launch_work).parameters) == ["n"]


def test_python_mirrors_the_kernels_geometry():
    from bitflood_amd import hashing
    hpp = open(os.path.join(CSRC, "hash_text.hpp")).read()
    assert "constexpr uint32_t kMapBlock = %d;" % hashing.HASH_TEXT_MAP_BLOCK in hpp
    assert "constexpr uint32_t kScanWidth = %d;" % hashing.HASH_TEXT_SCAN_WIDTH in hpp


@pytest.mark.parametrize("n", [0, 1, 1023, 1024, 1025, (1 << 31) - 1])
def test_work_is_the_documented_formula(lib, n):
    """include/lbf_hash.h: ((20 * n + 15) & ~15) + 4 * ceil(n / 1024)."""
    from bitflood_amd import verify_hashes_launch_work
    want = ((20 * n + 15) & ~15) + 4 * ((n + 1023) // 1024)
    assert lib.lbf_verify_hashes_launch_work(n) == want == verify_hashes_launch_work(n)
    assert want % 4 == 0 and want >= 20 * n
    assert "((20 * n + 15) & ~15) + 4 * ceil(n / 1024)" in open(_capi.HEADER_PATH).read()


def _tables(n=1):
    """Host arrays standing in for every table of the two calls (the refusals
    below come before any of them is read)."""
    return dict(data=np.zeros(64, np.uint8), off=np.zeros(n, np.uint64), size=np.full(n, 8, np.uint32),
                hashes=np.zeros(27 * n + 8, np.uint8), hoff=np.zeros(n, np.uint64), hlen=np.full(n, 27, np.uint32),
                cmap=np.zeros(n, np.uint8), miss=np.zeros(n, np.uint32), cnt=np.zeros(2, np.uint32),
                dig=np.zeros(20 * n + 4, np.uint8), work=np.zeros(32 * n + 16, np.uint8))


def _ptrs(t, null, shift):
    return {k: (None if k in null else v.ctypes.data + (shift or {}).get(k, 0)) for k, v in t.items()}


def _hashes(lib, t, n=1, null=(), shift=None):
    p = _ptrs(t, null, shift)
    return lib.lbf_sha1_hashes_launch(p["data"], p["off"], p["size"], n, p["hashes"], p["hoff"], p["dig"], p["work"],
                                      None)


def _verify(lib, t, n=1, null=(), shift=None):
    p = _ptrs(t, null, shift)
    return lib.lbf_verify_hashes_launch(p["data"], p["off"], p["size"], n, p["hashes"], p["hoff"], p["hlen"],
                                        p["cmap"], p["miss"], p["cnt"], p["dig"], p["work"], None)


@pytest.mark.parametrize("table", ["data", "off", "size", "hashes", "work"])
def test_hashes_launch_refuses_a_null_required_argument(lib, table):
    _refused(lib, _hashes(lib, _tables(), null=(table,)), HASHES, b"null")


@pytest.mark.parametrize("table", ["data", "off", "size", "hashes", "cmap", "work"])
def test_verify_launch_refuses_a_null_required_argument(lib, table):
    _refused(lib, _verify(lib, _tables(), null=(table,)), VERIFY, b"null")


def test_refuse_too_many_chunks(lib):
    _refused(lib, _hashes(lib, _tables(), n=1 << 31), HASHES, b"2^31-1")
    _refused(lib, _verify(lib, _tables(), n=1 << 31), VERIFY, b"2^31-1")


def test_verify_launch_refuses_half_a_pair(lib):
    _refused(lib, _verify(lib, _tables(), null=("hlen",)), VERIFY, b"hash_offsets and hash_lens go together")
    _refused(lib, _verify(lib, _tables(), null=("hoff",)), VERIFY, b"hash_offsets and hash_lens go together")
    _refused(lib, _verify(lib, _tables(), null=("cnt",)), VERIFY, b"missing and missing_count go together")
    _refused(lib, _verify(lib, _tables(), null=("miss",)), VERIFY, b"missing and missing_count go together")


@pytest.mark.parametrize("table,by", [("off", 4), ("size", 2), ("hoff", 4)])
def test_hashes_launch_refuses_a_misaligned_table(lib, table, by):
    _refused(lib, _hashes(lib, _tables(n=2), n=1, shift={table: by}), HASHES, b"not aligned to its element size")


@pytest.mark.parametrize("table,by", [("off", 4), ("size", 2), ("hoff", 4), ("hlen", 2), ("miss", 2), ("cnt", 1)])
def test_verify_launch_refuses_a_misaligned_table(lib, table, by):
    _refused(lib, _verify(lib, _tables(n=2), n=1, shift={table: by}), VERIFY, b"not aligned to its element size")


@pytest.mark.parametrize("table", ["dig", "work"])
def test_refuse_digests_or_work_off_four_bytes(lib, table):
    _refused(lib, _hashes(lib, _tables(), shift={table: 2}), HASHES, b"4-byte aligned")
    _refused(lib, _verify(lib, _tables(), shift={table: 2}), VERIFY, b"4-byte aligned")


def test_tables_are_checked_against_their_allocations():
    """check_fits needs a device allocation to refuse anything (tests/test_gpu_hash_text.py runs it); here, that
    every table of both calls is on the validator's list with its element size."""
    text = open(os.path.join(CSRC, UNIT)).read()
    assert text.count("lbf::tables_fit(who, tables)") == 2 and text.count("lbf::tables_aligned(who, tables)") == 2
    for row in ('{d_offsets, 8, n, "offsets", true}', '{d_sizes, 4, n, "sizes", true}',
                '{d_hash_offsets, 8, n, "hash_offsets", true}', '{d_digests, 20, n, "digests", false}',
                '{d_work, 1, ht::work_bytes(n), "work", false}'):
        assert text.count(row) == 2, row
    for row in ('{d_hash_lens, 4, n, "hash_lens", true}', '{d_chunkmap, 1, n, "chunkmap", false}',
                '{d_missing, 4, n, "missing", true}', '{d_missing_count, 4, 1, "missing_count", true}'):
        assert text.count(row) == 1, row
    assert text.count('{d_hash_offsets ? nullptr : d_hashes, ht::kHashChars, n, "hashes", false}') == 2


def test_no_chunks_is_ok_with_every_pointer_null(lib):
    assert lib.lbf_sha1_hashes_launch(None, None, None, 0, None, None, None, None, None) == 0
    assert lib.lbf_verify_hashes_launch(None, None, None, 0, None, None, None, None, None, None, None, None,
                                        None) == 0
    t = _tables()
    t["cnt"][:] = 0xABCD
    assert _verify(lib, t, n=0, null=("hlen", "miss")) == 0
    assert (t["cnt"] == 0xABCD).all()  # *d_missing_count is not written


@needs_hipcc
def test_the_new_source_holds_exactly_the_four_kernels():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_digest
    got = isa_digest.digests(os.path.join(CSRC, UNIT))
    assert len(got) == 4, sorted(got)
    for k in KERNELS:
        assert sum(k in name for name in got) == 1, (k, sorted(got))
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert UNIT in srcs


@pytest.fixture(scope="module")
def remarks(tmp_path_factory):
    out = tmp_path_factory.mktemp("hash_text") / "k.o"
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


def test_alphabet_and_scan_come_from_the_shared_header():
    text = open(os.path.join(CSRC, UNIT)).read()
    assert '#include "b64_device.hpp"' in text
    code = re.sub(r"//[^\n]*", "", text)
    for call in ("b64d::fill_alphabet(", "b64d::chars_whole(", "b64d::chars_last(", "b64d::wg_exclusive_scan<"):
        assert call in code, call
    # no alphabet table of its own, in any spelling: no run of the alphabet's letters, no __constant__
    assert "__constant__" not in code
    assert not re.search(r"ABCDEFGH|abcdefgh|01234567", code)
    assert not re.search(r"'A' \+|'a' \+|'0' \+", code)
    assert len(re.findall(r"__global__", code)) == 4

"""The resumable base64 encode (lbf_b64_enc_state), the parts that need no GPU:
its rule (tests/wire_encode_model.py) against the whole texts of
tests/wire_layouts.xmlrpc_text (pinned to xmlrpc++'s recorded encoder output)
and base64.b64encode at every cut; the host entry points; the geometry the model
restates; the kernel's resource usage on gfx950; and the batch call's planner
(bitflood_amd/csrc/b64_encode_plan.hpp, by tests/c/b64_encode_plan_tests.cpp,
plain and under ASan/UBSan as stand-alone programs)."""
import base64
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_encode_model as E
from tests import wire_layouts as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def whole(data: bytes, layout: int) -> bytes:
    return W.xmlrpc_text(data) if layout == E.XMLRPC else base64.b64encode(data)


def run_pieces(pieces, layout):
    """The pieces through the model, the last one final: the slot they fill."""
    size = sum(len(p) for p in pieces)
    slot = bytearray(b"\xEE" * (E.text_length(size, layout) + 3))
    state, end = E.init(layout), 0
    for k, p in enumerate(pieces):
        last = k == len(pieces) - 1
        state, at, chars, length = E.update(state, p, last)
        assert at == end, (k, at, end)  # pieces' characters follow one another without a gap
        assert slot[at:at + len(chars)] == b"\xEE" * len(chars)
        slot[at:at + len(chars)] = chars
        end = at + len(chars)
        if last:
            assert length == end == E.text_length(size, layout)
        else:
            sofar = b"".join(pieces[:k + 1])
            taken = len(sofar)
            assert state == (taken, sofar[taken - taken % 3:], taken % 3, layout)
            assert end == E.pos(taken // 3, layout)
    assert state == E.init(layout)
    assert slot[end:] == b"\xEE\xEE\xEE"
    return bytes(slot[:end])


# ------------------------------------------------------------ 1. the rule
@pytest.mark.parametrize("layout", (E.XMLRPC, E.FLAT))
def test_model_gives_the_whole_text_at_every_cut(layout):
    """167 bytes: three lines and a 5-byte tail -- every ncarry, a cut on each
    side of two separators, and a final "xxx="."""
    d = W.chunk_bytes(167)
    want = whole(d, layout)
    assert len(want) == E.text_length(167, layout) == (3 * 73 + 8 if layout == E.XMLRPC else 224)
    assert want.endswith(b"=") and not want.endswith(b"==")
    for a in range(168):
        assert run_pieces([d[:a], d[a:]], layout) == want, a
    # three pieces, the middle one shorter than a group: the carry is topped up from what was carried
    for a in range(0, 167, 5):
        for m in (0, 1, 2):
            assert run_pieces([d[:a], d[a:a + m], d[a + m:]], layout) == want, (a, m)


@pytest.mark.parametrize("layout", (E.XMLRPC, E.FLAT))
@pytest.mark.parametrize("size", (0, 1, 2, 3, 53, 54, 55, 108, 110))
def test_model_final_sizes(size, layout):
    d = W.chunk_bytes(size)
    want = whole(d, layout)
    for a in range(size + 1):
        assert run_pieces([d[:a], d[a:]], layout) == want, a
        assert run_pieces([d[:a], d[a:], b""], layout) == want, a  # an empty final piece
    if size == 54 and layout == E.XMLRPC:
        assert len(want) == 73 and want[-1:] == b" "  # the chunk ends with its separator


def test_text_length_and_state_init():
    """lbf_b64_text_length and lbf_b64_enc_state_init: host code, no GPU."""
    import bitflood_amd
    from bitflood_amd import B64_ENC_STATE_DTYPE, hashing, new_b64_enc_states
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in ("lbf_b64_enc_state_init", "lbf_b64_text_length", "lbf_b64_encode_update_launch",
              "lbf_b64_encode_update_batch"):
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s
    assert {"B64_ENC_STATE_DTYPE", "new_b64_enc_states", "b64_text_length", "b64_encode_update_launch"} <= set(
        hashing.__all__)
    assert hasattr(hashing.ChunkHasher, "update_encode") and callable(bitflood_amd.b64_encode_update_launch)
    for size in range(401):
        d = W.chunk_bytes(size)
        assert lib.lbf_b64_text_length(size, 0) == lib.lbf_b64_put_length(size) == len(W.xmlrpc_text(d)), size
        assert lib.lbf_b64_text_length(size, 1) == len(base64.b64encode(d)), size
        assert hashing.b64_text_length(size, "xmlrpc") == E.text_length(size, E.XMLRPC)
        assert hashing.b64_text_length(size, "flat") == E.text_length(size, E.FLAT)
    assert lib.lbf_b64_text_length(1 << 30, 0) == E.MAX_TEXT_CAP
    assert B64_ENC_STATE_DTYPE.itemsize == 16
    for name, layout in (("xmlrpc", 0), ("flat", 1)):
        st = new_b64_enc_states(3, name)
        assert st.tobytes() == (bytes(13) + bytes([layout]) + bytes(2)) * 3
        assert (st["taken"] == 0).all() and (st["layout"] == layout).all()
    raw = np.full(32, 0xAB, dtype=np.uint8)
    lib.lbf_b64_enc_state_init(raw.ctypes.data, 2, 7)  # anything but FLAT is XMLRPC
    assert raw.tobytes() == bytes(32)
    with pytest.raises(ValueError):
        new_b64_enc_states(1, "lines")
    header = open(_capi.HEADER_PATH).read()
    assert "#define LBF_B64_LAYOUT_XMLRPC 0" in header and "#define LBF_B64_LAYOUT_FLAT   1" in header


def test_model_geometry_is_the_sources():
    text = open(os.path.join(CSRC, "b64_encode_update.hpp")).read()

    def const(name):
        return int(re.search(r"\b%s = (\d+)" % name, text).group(1))
    assert (const("kLineGroups"), const("kLineBytes"), const("kLineChars")) == (E.LINE_GROUPS, E.LINE_BYTES,
                                                                                   E.LINE_CHARS)
    assert const("kEncUpdLines") == E.TILE_LINES == W.ENC_LINES
    assert "kEncUpdTileBytes = kEncUpdLines * kLineBytes" in text and E.TILE_BYTES == 6048
    assert "kEncUpdTileText = kEncUpdLines * kLineChars" in text and E.TILE_TEXT == 8176
    assert "kEncUpdTileFlat = kEncUpdTileGroups * 4" in text and E.TILE_FLAT == 8064
    assert "kEncMaxChunk = 1ull << 30" in text and "kEncMaxTaken = 1ull << 61" in text
    assert "return flat ? 4 * g : 4 * g + g / kLineGroups" in text
    assert "kSeparator = ' '" in text
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert "b64_encode_update.hip" in srcs and "b64_encode_batch.cpp" in srcs


# ------------------------------------------------------------ 2. the kernel's resources
@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_encode_update_kernel_has_no_scratch_and_no_spills(tmp_path):
    """Two kernels; nothing in scratch, nothing spilled; at most 64 VGPRs; LDS for
    two staged tiles and the alphabet, eight workgroups to a CU and more."""
    src = os.path.join(CSRC, "b64_encode_update.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-S", "-o", str(tmp_path / "e.s"),
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks}
    assert len(kernels) == 2, sorted(kernels)
    assert sum("b64_encode_update_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert sum("b64_encode_sizes_kernel" in k for k in kernels) == 1, sorted(kernels)
    for name, rem in kernels.items():
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
        assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
        assert re.search(r"Dynamic Stack: False", rem), rem
        assert int(re.search(r" VGPRs: (\d+)", rem).group(1)) <= 64, rem
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", rem).group(1))
        if "b64_encode_update_kernel" in name:
            assert 2 * E.TILE_BYTES <= lds <= 20480, lds
        else:
            assert lds == 0
    # the code object's own metadata says the same
    meta = open(tmp_path / "e.s").read()
    meta = meta[meta.index(".amdgpu_metadata"):]
    assert len(re.findall(r"\.private_segment_fixed_size:\s*0\b", meta)) == 2, meta[:2000]
    assert len(re.findall(r"\.private_segment_fixed_size:", meta)) == 2
    assert re.findall(r"\.vgpr_spill_count:\s*(\d+)", meta) == ["0", "0"]
    assert re.findall(r"\.sgpr_spill_count:\s*(\d+)", meta) == ["0", "0"]
    text = open(src).read() + open(os.path.join(CSRC, "b64_device.hpp")).read()  # the kernel and its shared helpers
    assert "asm" not in text.replace("__launch_bounds__", "")  # no inline assembly, and only barriers synchronise
    assert "while (" not in text and "__syncthreads()" in text


# ------------------------------------------------------------ 3. the planner
def _build_plan_tests(tmp_path, name, extra):
    exe = str(tmp_path / name)
    cc = subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", *extra,
                         "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                         os.path.join(ROOT, "tests", "c", "b64_encode_plan_tests.cpp"), "-o", exe],
                        capture_output=True, text=True)
    assert cc.returncode == 0, cc.stderr[-3000:]
    return exe


@pytest.mark.parametrize("name,extra", [("plain", []),
                                        ("asan_ubsan", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"])])
def test_b64_encode_plan_program(tmp_path, name, extra):
    """Every refusal, the cut of an oversized piece, the characters a cut writes,
    device places and the run merging of the copy back, as a stand-alone program
    (no preload, no Python under a sanitizer)."""
    exe = _build_plan_tests(tmp_path, "b64_encode_plan_tests_" + name, extra)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "UBSAN_OPTIONS": "halt_on_error=1:print_stacktrace=1"})
    assert r.returncode == 0, r.stdout + r.stderr[-3000:]
    assert r.stdout.splitlines()[-1] == "b64_encode_plan_tests: OK", r.stdout


def test_b64_encode_plan_header_is_hip_free():
    for name in ("b64_encode_plan.hpp", "b64_encode_update.hpp"):
        text = open(os.path.join(CSRC, name)).read()
        assert "hip_runtime" not in text and "hipStream" not in text and "getenv" not in text, name

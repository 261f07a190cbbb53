"""The one-shot wire encode in either layout, without a GPU: the two entry
points (lbf_verify_encode_b64_layout_batch, lbf_verify_encode_b64_launch) exist
and refuse what they can refuse before any HIP call, and
tests/wire_flat_encode_model.py states the kernel's geometry and the text
lengths as the library does."""
import os
import re

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_flat_encode_model as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
GIB = 1 << 30


@pytest.fixture(scope="module")
def lib():
    return _capi.load()


def _refused(lib, rc, *words):
    msg = lib.lbf_last_error() or b""
    assert rc == _capi.LBF_ERR_INVALID, (rc, msg)
    for w in words:
        assert w in msg, (w, msg)


def test_both_symbols_load(lib):
    for name in ("lbf_verify_encode_b64_layout_batch", "lbf_verify_encode_b64_launch"):
        assert name in _capi._SIGS and name in _capi.header_symbols()
        assert getattr(lib, name).argtypes == _capi._SIGS[name][1]
    assert lib.lbf_abi_version() == 1


def _tables(n=1, size=100):
    """Host arrays standing in for every table of either call (the refusals
    below come before any of them is read)."""
    return dict(data=np.zeros(256, np.uint8), off=np.zeros(n, np.uint64), size=np.full(n, size, np.uint32),
                exp=np.zeros(20 * n, np.uint8), ver=np.zeros(n, np.uint8), dig=np.zeros(20 * n, np.uint8),
                text=np.zeros(512, np.uint8), toff=np.zeros(n, np.uint64))


def _launch(lib, t, layout=F.FLAT, max_size=100, n=1, **null):
    p = {k: (None if null.get(k) else v.ctypes.data) for k, v in t.items()}
    return lib.lbf_verify_encode_b64_launch(p["data"], p["off"], p["size"], n, max_size, p["dig"], p["exp"], p["ver"],
                                            layout, p["text"], p["toff"], None)


def _batch(lib, t, layout=F.FLAT, n=1, ctx=None, **null):
    p = {k: (None if null.get(k) else v.ctypes.data) for k, v in t.items()}
    return lib.lbf_verify_encode_b64_layout_batch(ctx, p["data"], t["data"].size, p["off"], p["size"], n, p["exp"],
                                                  p["ver"], layout, p["text"], t["text"].size, p["toff"])


@pytest.mark.parametrize("table", ["data", "off", "size", "text", "toff"])
def test_launch_refuses_a_null_table(lib, table):
    _refused(lib, _launch(lib, _tables(), **{table: True}), b"lbf_verify_encode_b64_launch", b"null")


@pytest.mark.parametrize("layout", [2, -1, 256])
def test_launch_refuses_an_unknown_layout(lib, layout):
    _refused(lib, _launch(lib, _tables(), layout=layout), b"lbf_verify_encode_b64_launch", b"layout")


def test_launch_refuses_a_max_size_over_1_gib(lib):
    for layout in (F.XMLRPC, F.FLAT):
        rc = _launch(lib, _tables(), layout=layout, max_size=GIB + 1)
        _refused(lib, rc, b"lbf_verify_encode_b64_launch", b"1 GiB")


def test_launch_of_no_chunks_is_ok_and_needs_no_tables(lib):
    assert lib.lbf_verify_encode_b64_launch(None, None, None, 0, 0, None, None, None, F.FLAT, None, None, None) == 0
    # the layout and max_size are looked at all the same
    _refused(lib, _launch(lib, _tables(), layout=2, n=0), b"layout")
    _refused(lib, _launch(lib, _tables(), max_size=GIB + 1, n=0), b"1 GiB")


@pytest.mark.parametrize("table", ["data", "off", "size", "exp", "ver", "text", "toff"])
def test_batch_refuses_a_null_table(lib, table):
    _refused(lib, _batch(lib, _tables(), **{table: True}), b"lbf_verify_encode_b64_layout_batch", b"null argument")


@pytest.mark.parametrize("layout", [2, -1, 256])
def test_batch_refuses_an_unknown_layout(lib, layout):
    _refused(lib, _batch(lib, _tables(), layout=layout), b"lbf_verify_encode_b64_layout_batch", b"layout")


def test_batch_without_a_context_is_refused(lib):
    """No GPU here, so no context: with every table in place the call stops at
    the context, before it looks at a size (the 1 GiB bound on a chunk is the
    GPU tests')."""
    _refused(lib, _batch(lib, _tables()), b"null context")


def test_model_text_lengths_are_the_librarys(lib):
    sizes = list(range(201)) + [F.T + d for d in (-3, -2, -1, 0, 1, 2, 3)] + [F.K * F.T + d for d in (-1, 0, 1)]
    for layout in (F.XMLRPC, F.FLAT):
        for s in sizes:
            assert F.text_length(s, layout) == lib.lbf_b64_text_length(s, layout), (s, layout)
            assert F.text_length(s, layout) == len(F.text(bytes(s), layout)), (s, layout)
    for s in sizes:
        assert F.text_length(s, F.XMLRPC) == lib.lbf_b64_put_length(s)


def test_model_geometry_is_the_kernels():
    """T and K as the header's defaults and the kernel's static_assert state them."""
    hpp = open(os.path.join(CSRC, "b64_flat_encode.hpp")).read()
    hip = open(os.path.join(CSRC, "b64_flat_encode.hip")).read()
    groups = int(re.search(r"#define LBF_B64_FLAT_ENC_TILE_GROUPS (\d+)", hpp).group(1))
    per = int(re.search(r"#define LBF_B64_FLAT_ENC_TILES_PER_GROUP (\d+)", hpp).group(1))
    assert (3 * groups, per) == (F.T, F.K) and F.TILE_TEXT == 4 * groups
    m = re.search(r"static_assert\(kTileBytes == (\d+) && kTileText == (\d+) && kTilesPerGroup == (\d+),", hip)
    assert m and tuple(int(x) for x in m.groups()) == (F.T, F.TILE_TEXT, F.K)
    assert "constexpr uint32_t kPerLaunch = %d;" % F.CHUNKS_PER_LAUNCH in hip
    assert F.T % 48 == 0  # bytes and text of a tile are whole 16-byte blocks


def test_test_sizes_reach_every_path():
    """The GPU tests' sizes: all three forms of the last group below and above
    one block, one line, one tile and one workgroup, and a chunk of two
    workgroups, a tile and one byte: its last tile holds one padded group."""
    s = set(F.sizes_for(F.FLAT))
    assert {0, 1, 2, 3, 11, 12, 13, 53, 54, 55} <= s
    for edge in (F.T, F.K * F.T):
        assert {edge - 1, edge, edge + 1, edge + 2} <= s
        assert {x % 3 for x in (edge - 1, edge, edge + 1)} == {0, 1, 2}
    big = max(s)
    assert -(-F.text_length(big, F.FLAT) // F.TILE_TEXT) == 2 * F.K + 2
    assert set(F.sizes_for(F.XMLRPC)) > s


def test_header_keeps_the_abi_version():
    text = open(_capi.HEADER_PATH).read()
    assert re.search(r"#define LBF_ABI_VERSION 1\b", text)
    for name in ("lbf_verify_encode_b64_layout_batch", "lbf_verify_encode_b64_launch"):
        assert len(re.findall(r"\bint %s\(" % name, text)) == 1


def test_python_helpers_take_a_layout():
    import inspect

    from bitflood_amd import ChunkHasher, verify_encode_b64_launch
    assert inspect.signature(ChunkHasher.verify_encode_b64).parameters["layout"].default == "xmlrpc"
    p = inspect.signature(verify_encode_b64_launch).parameters
    assert list(p)[:8] == ["base", "offsets", "sizes", "n", "max_size", "text", "text_offsets", "layout"]
    assert p["layout"].default == "xmlrpc"
    assert all(p[k].default is None for k in ("digests", "expected", "verdicts", "stream"))

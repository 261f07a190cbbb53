"""The one-shot flat encode's geometry and its expected values -- TEST
INFRASTRUCTURE, no GPU, no pytest.

b64_flat_encode_kernel (bitflood_amd/csrc/b64_flat_encode.hip) lays tiles of
T bytes (4 * T / 3 characters) over a chunk, K consecutive tiles per
workgroup.  The sizes the GPU tests draw stand on both sides of every place
where the kernel takes another path: the last group's three forms, one line
of xmlrpc++'s layout (54 bytes), one tile, one workgroup, and a chunk of two
workgroups, a tile and one byte.  tests/test_b64_flat_encode_cpu.py reads T and K back from
the source.

Expected texts come from outside the code under test: base64.b64encode for
unbroken text, tests/wire_layouts.xmlrpc_text (pinned to xmlrpc++'s recorded
encoder output) for lines.
"""
import base64

from tests import wire_layouts as W

T = 6144  # tile bytes: 2,048 groups -> 8,192 characters, 512 blocks of 16
K = 1     # tiles per workgroup
TILE_TEXT = 4 * T // 3
CHUNKS_PER_LAUNCH = 65535  # grid.y of one launch
XMLRPC, FLAT = 0, 1        # LBF_B64_LAYOUT_*
LAYOUTS = {"xmlrpc": XMLRPC, "flat": FLAT}

SMALL_SIZES = (0, 1, 2, 3, 4, 5, 6, 11, 12, 13, 47, 48, 49, 53, 54, 55)
TILE_SIZES = (T - 1, T, T + 1, T + 2, K * T - 1, K * T, K * T + 1, K * T + 2, 2 * K * T + T + 1)


def text_length(size: int, layout: int) -> int:
    """Characters of the whole text of `size` bytes: four per group of three
    bytes, the last group padded; in lines, a separator after every 18th
    complete group."""
    groups = (size + 2) // 3
    return 4 * groups + (size // 3 // 18 if layout == XMLRPC else 0)


def text(data: bytes, layout: int) -> bytes:
    return W.xmlrpc_text(data) if layout == XMLRPC else base64.b64encode(data)


def sizes_for(layout: int) -> list:
    """Test 1's chunk sizes; for lines, those of wire_layouts.encode_cases() too."""
    sizes = list(SMALL_SIZES + TILE_SIZES)
    if layout == XMLRPC:
        sizes += sorted({s for s, _, _ in W.encode_cases()})
    return sizes

"""The fixed slice of the random piecewise and launch scenes on the GPU, and the
two deterministic scenes that go with it.

tests/piece_cases.py draws the scenes and holds everything a call must give,
from the CPU models alone; tests/test_piece_cases.py proves on the CPU what the
slice reaches; tests/piece_driver.py feeds a scene to the library call by call,
each call through the route and under the (lines, flat, fused) switches the
scene drew for it, resuming the records the call before it left, and checks
every call whole.  A failure names the seed, the call, the route, the switches
and the chain, and the line that replays it (tools/fuzz_pieces.py draws fresh
seeds from the same generator).
"""
import pytest

from bitflood_amd import _capi
from bitflood_amd import hashing as H
from tests import piece_cases as P
from tests.piece_driver import Runner, run_scene

pytestmark = pytest.mark.gpu

GROUPS = [(fam, seeds[i:i + P.GROUP]) for fam, seeds in P.SLICE.items() for i in range(0, len(seeds), P.GROUP)]


@pytest.fixture
def switches_back():
    """Whatever a scene does, the process leaves with the switches it came with."""
    before = (H.set_b64_lines(1), H.set_b64_flat(0), H.set_b64_fused(0))
    H.set_b64_lines(before[0]), H.set_b64_flat(before[1]), H.set_b64_fused(before[2])
    yield
    assert (H.set_b64_lines(before[0]), H.set_b64_flat(before[1]), H.set_b64_fused(before[2])) == before


@pytest.mark.parametrize("family,seeds", GROUPS, ids=[f"{fam}-{seeds[0]}..{seeds[-1]}" for fam, seeds in GROUPS])
def test_slice(hasher, switches_back, family, seeds):
    """GROUP scenes of one family; every seed of the slice is run, none is skipped."""
    for seed in seeds:
        scene = P.case(seed)
        assert scene.family == family and scene.calls
        run_scene(hasher, scene)


# ------------------------------------------- every bit of the expected digest decides
VARIANTS = [1, 7, 10, 11, 12]  # the shipped kernels, as tests/test_gpu_parity.py names them


@pytest.fixture(params=VARIANTS, ids=lambda v: {1: "lane", 7: "pc4b64", 10: "pcx5", 11: "lds2", 12: "pc4x2"}[v])
def variant(request):
    H.set_kernel_variant(request.param)
    yield request.param
    H.set_kernel_variant(0)


def _bits(hasher, route, layout="xmlrpc"):
    scene = P.bits_scene(route, layout)
    r = Runner(hasher, scene)
    got = r.run(0)
    P.check(scene, 0, got)
    finals = [i for i, f in enumerate(scene.calls[0].final) if f]
    assert got["verdicts"][finals].tolist() == [0] * P.BITS + [1] * P.BITS_RIGHT


@pytest.mark.parametrize("route", ["uniform_launch", "batch_launch"])
def test_every_digest_bit_decides_the_verdict_one_shot(hasher, variant, route):
    """192 tiny chunks, chunk k < 160 with bit k of its expected digest wrong:
    the verdicts are 160 zeros and 32 ones under every shipped kernel (the
    compare of kern_lane.hpp and of kern_common.hpp's write_result)."""
    _bits(hasher, route)


@pytest.mark.parametrize("route", ["update_launch", "update_seq_launch"])
def test_every_digest_bit_decides_the_verdict_final_pieces(hasher, route):
    """The same on final pieces (sha1_resume.hpp's write_final)."""
    _bits(hasher, route)


@pytest.mark.parametrize("layout", P.LAYOUTS)
@pytest.mark.parametrize("route", ["b64_update_launch", "b64_encode_update_launch", "verify_b64_launch",
                                   "verify_encode_b64_launch"])
def test_every_digest_bit_decides_the_verdict_composites(hasher, route, layout):
    """The same behind the four composite launches, whose own kernels clear or
    keep the hash's verdict: the lengths all fit, so nothing but the bit decides."""
    _bits(hasher, route, layout)


# ------------------------------------- the 16 K-32 K selection behind the wire kernels
@pytest.mark.parametrize("route", P.ROUTES["shot"])
def test_wire_launches_behind_the_16k_32k_selection(hasher, route):
    """16,390 chunks of 3..55 bytes, mixed layouts, a few wrong digests and a
    few damaged texts: the composite's hash stage runs pc4x2, which no other
    test puts behind a decode or in front of an encode.  Checked whole."""
    assert _capi.load().lbf_get_kernel_variant() == 0 and _capi.load().lbf_kernel_for(P.SELECTION_CHUNKS) == 12
    scene = P.selection_scene(route)
    assert run_scene(hasher, scene) == len(scene.calls) > 0

"""libBitFlood::PieceHasher::UpdateEncode on the GPU: the C++ test program
bitflood_amd/host/encode_piece_tests.cpp (built by bitflood_amd/host/Makefile)
feeds three slots, both text layouts, in pieces over two calls, and compares the
text with strings computed on the host; Reset in mid-chunk and the refusals are
in it too."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_piece_hasher_update_encode():
    out = subprocess.run([os.path.join(ROOT, "bitflood_amd", "lib", "lbf_encode_piece_tests")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "encode_piece_tests OK" in out.stdout

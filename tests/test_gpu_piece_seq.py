"""libBitFlood::PieceHasher::UpdateSeq and UpdateTextSeq on the GPU: the C++
program bitflood_amd/host/seq_piece_tests.cpp (built by build()) drives three
slots with several pieces each in one call, as bytes and as text, against the
hash strings of tests/golden/kat.json."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cpp_piece_hasher_seq():
    out = subprocess.run([os.path.join(ROOT, "bitflood_amd", "lib", "lbf_seq_piece_tests")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "seq_piece_tests OK" in out.stdout

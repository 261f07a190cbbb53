"""The base64 translation units beside sha1_kernels.hip keep their recorded
gfx950 instruction streams (CPU only: hipcc cross-compiles).

tests/golden/isa_b64.json holds per-kernel digests of every kernel of these
sources, recorded before their device helpers moved into
bitflood_amd/csrc/b64_device.hpp (tools/isa_digest.py --record, several
sources).  A refactor that moves code between headers leaves them unchanged;
a change to a kernel re-records its source on purpose.  The shipped hash and
one-shot wire kernels are pinned the same way by tests/test_isa.py.
"""
import json
import os
import shutil
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
GOLDEN = os.path.join(ROOT, "tests", "golden", "isa_b64.json")
SOURCES = ["b64_update.hip", "b64_update_lines.hip", "b64_flat.hip", "b64_update_fused.hip", "b64_update_seq.hip",
           "b64_encode_update.hip", "b64_flat_encode.hip"]

pytestmark = pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")


def test_every_base64_source_is_recorded():
    recorded = json.load(open(GOLDEN))
    assert sorted(recorded["sources"]) == sorted("bitflood_amd/csrc/" + s for s in SOURCES)
    assert recorded["hipcc_flags"] == ["--offload-arch=gfx950", "-O3", "-std=c++17"]
    for kernels in recorded["sources"].values():
        assert kernels and all(k["instructions"] > 0 and len(k["sha256"]) == 64 for k in kernels.values())


@pytest.mark.parametrize("source", SOURCES)
def test_base64_kernel_isa_matches_recorded_digests(source):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import isa_digest
    rel = "bitflood_amd/csrc/" + source
    want = json.load(open(GOLDEN))["sources"][rel]
    got = isa_digest.digests(os.path.join(ROOT, rel))
    assert sorted(got) == sorted(want)
    for k in want:
        assert got[k] == want[k], (source, k)

"""C5 with a seeder that encodes on the GPU in the Java and Perl peers' layout:
`lbf_loopback --synthetic --gpu-encode --wire-layout flat`, the seeder's verify
and its unbroken base64 in one call (Flood::VerifyEncodeChunks with
LBF_B64_LAYOUT_FLAT, b64_flat_encode_kernel).  Two processes
(tests/c5_pair.py); the leecher decodes and verifies on the GPU as before."""
import pytest

from tests.c5_pair import run_pair

pytestmark = pytest.mark.gpu

CHUNKS, CHUNK, TAIL = 64, 65536, 12345


def test_gpu_flat_seeder_and_one_corrupted_chunk(tmp_path, monkeypatch):
    """64 chunks of 64 KiB and a ragged tail; chunk 63 leaves the seeder with a
    flipped character on its first send: it is rejected once, asked for again
    and accepted, and the file arrives whole.  With the leecher's flat pass on,
    every frame went through it: the text on the wire is unbroken."""
    monkeypatch.setenv("LBF_B64_FLAT", "1")
    opts = ["--size", str(CHUNKS * CHUNK + TAIL), "--chunksize", str(CHUNK), "--window", "32", "--batch", "16",
            "--corrupt", str(CHUNKS), "--synthetic", "--gpu-encode", "--wire-layout", "flat"]
    r, seeder, leecher = run_pair(opts, str(tmp_path / "c5"), timeout=300)
    assert r["resume_verify_complete"] and r["files_identical"]
    assert r["chunks"] == CHUNKS + 1
    for line in (seeder, leecher):
        assert line["gpu_encode"] is True and line["wire_layout"] == "flat"
    assert r["corrupted_sent"] == 1 and r["leecher"]["rejected"] == 1 and r["leecher"]["undecodable"] == 0
    assert r["leecher"]["flat_chunks"] == CHUNKS + 2    # every frame, the corrupted one included
    assert r["pids"]["seeder"] != r["pids"]["leecher"]

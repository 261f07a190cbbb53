"""C5 with a seeder that frames chunks as a Java or Perl peer would: unbroken
base64, no line separators (`lbf_loopback --wire-layout flat`, a host-side
encode).  Two processes (tests/c5_pair.py): the leecher decodes and verifies
on the GPU through Flood::VerifyTextChunks, and with LBF_B64_FLAT=1 every
frame is a candidate of the flat pass (bitflood_amd/csrc/b64_flat.hip)."""
import pytest

from tests.c5_pair import run_pair

pytestmark = pytest.mark.gpu

CHUNKS, CHUNK = 64, 262144


@pytest.mark.parametrize("switch,flat_chunks", [("1", CHUNKS + 1), ("0", 0)])
def test_flat_seeder_and_one_corrupted_chunk(tmp_path, monkeypatch, switch, flat_chunks):
    """64 chunks of 256 KiB, the last one corrupted on its first send: it is
    rejected, asked for again and accepted, and the file arrives whole.  With
    the switch on the leecher's flat pass decoded every frame, the corrupted one
    included (a flipped byte leaves the text flat); with it off, none -- and the
    same verdicts."""
    monkeypatch.setenv("LBF_B64_FLAT", switch)
    opts = ["--size", str(CHUNKS * CHUNK), "--chunksize", str(CHUNK), "--window", "32", "--batch", "16",
            "--corrupt", str(CHUNKS), "--wire-layout", "flat"]
    r, seeder, leecher = run_pair(opts, str(tmp_path / "c5"), timeout=300)
    assert r["resume_verify_complete"] and r["files_identical"]
    assert r["wire_layout"] == "flat" and r["gpu_decode"] is True and r["chunks"] == CHUNKS
    assert r["corrupted_sent"] == 1 and r["leecher"]["rejected"] == 1 and r["leecher"]["undecodable"] == 0
    assert r["leecher"]["flat_chunks"] == flat_chunks
    assert r["pids"]["seeder"] != r["pids"]["leecher"]

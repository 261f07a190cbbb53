"""The flat path of the base64 decode (unbroken RFC 4648 text, as bitflood's
Java and Perl peers frame a chunk), the parts that need no GPU: its rule
(tests/wire_flat_model.py) against the general rule (tests/wire_piece_model.update
and tests/wire_layouts.decode, both pinned to xmlrpc++'s recorded answers) at
every cut of unbroken texts, next to every kind of damage and on the encoder's
own layout; the new entry points; and the two kernels' resource usage on gfx950."""
import base64
import binascii
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_flat_model as F
from tests import wire_layouts as W
from tests import wire_line_model as L
from tests import wire_piece_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
SIZES = (0, 1, 2, 3, 55, 57, 58, 864)


def check_rest(state, rest: bytes, what):
    """Both forms of the model's prefix of `rest` against the general rule;
    returns (the longest prefix, the tiled one)."""
    taken = []
    for tiles in (False, True):
        n, body, after = F.take(state, rest, tiles=tiles)
        assert 0 <= n <= len(rest), what
        want_state, want = M.update(state, rest[:n])
        assert body == want and after == want_state, (what, tiles, n)
        v = M.TABLE[np.frombuffer(rest[:n], dtype=np.uint8)]
        assert (v < M.EQ).all(), (what, tiles, n)  # alphabet characters only: no '=', nothing skipped
        if n == 0:
            assert after == state, what  # nothing taken: the carry, if any, stays for the general rule
        else:
            assert len(after[1]) == 0 and not after[2] and after[0] % 3 == 0, what
        taken.append(n)
    assert taken[1] <= taken[0], what  # the kernel's tiles give up whole tiles, never take more
    return tuple(taken)


# ------------------------------------------------------------ 1. the piecewise rule
@pytest.mark.parametrize("size", SIZES)
def test_prefix_is_the_general_rule_at_every_cut_of_unbroken_text(size):
    """Both pieces of every two-way cut: the prefix decodes by places to what
    the general rule gives, leaves nothing carried, and of an undamaged text
    leaves at most three characters of an unfinished group and the '=' group."""
    d = W.chunk_bytes(size)
    t = F.text(d)
    assert len(t) == F.flat_len(size) and W.decode(t) == d
    for a in range(len(t) + 1):
        n1, n1t = check_rest(M.init(), t[:a], (size, a, 1))
        assert n1 == n1t and a - n1 <= 7, (size, a, n1)
        state, _ = M.update(M.init(), t[:a])
        if state[2]:
            assert F.take(state, t[a:])[0] == 0  # the data has ended: nothing for the flat path
            continue
        n2, n2t = check_rest(state, t[a:], (size, a, 2))
        assert n2 == n2t, (size, a)
        if len(t) - a >= 4 - len(state[1]) or not state[1]:
            assert len(t) - a - n2 <= 7, (size, a, n2)
        else:
            assert n2 == 0  # fewer characters than complete the carried group


def test_tiles_follow_the_chunk_not_the_piece():
    """A junk character in tile 1 of the chunk: the tiled prefix of a piece that
    starts in tile 0 ends at the chunk's tile edge, wherever the piece began."""
    d = W.chunk_bytes(3 * F.TILE_BYTES)
    t = bytearray(F.text(d))
    t[F.TILE_TEXT + 100] = ord("*")
    t = bytes(t)
    for a in (0, 1, 2, 3, 4, 999, F.TILE_TEXT - 5, F.TILE_TEXT - 4, F.TILE_TEXT, F.TILE_TEXT + 3):
        state, _ = M.update(M.init(), t[:a])
        n, nt = check_rest(state, t[a:], a)
        assert a + n == F.TILE_TEXT + 100  # the whole groups in front of the damage
        assert a + nt == (F.TILE_TEXT if a < F.TILE_TEXT else a + (4 - len(state[1])) % 4), (a, nt)


@pytest.mark.parametrize("kind", W.KINDS)
def test_prefix_next_to_damage(kind):
    """Every kind of damage at every place of the unbroken texts, each cut two
    characters before its damage: the second piece's prefix holds only
    alphabet characters and by places decodes to what the general rule gives;
    and one-shot, a damaged text is decoded flat only when its bytes by places
    are the general rule's."""
    short = flat = 0
    for size in SIZES:
        t0 = F.text(W.chunk_bytes(size))
        for p in W.positions(len(t0), kind):
            t = W.damage(t0, kind, p)
            a = max(p - 2, 0)
            state, _ = M.update(M.init(), t[:a])
            if not state[2]:
                n, _ = check_rest(state, t[a:], (kind, size, p))
                short += n < len(t) - a - 7
            if F.decoded_flat(t, size):
                flat += 1
                assert base64.b64decode(t, validate=True) == W.decode(t), (kind, size, p)
            elif F.is_candidate(len(t), size):
                with pytest.raises(binascii.Error):  # what is not flat is not RFC 4648 text either
                    base64.b64decode(t, validate=True)
    # damage stops the prefix somewhere; a cut text just ends, and an alphabet character more, less or changed
    # is no damage to this path
    assert short > 0 or kind in ("cut", "alpha", "ins_alpha", "drop")
    # only another alphabet character, '=' over the last group's padding places, or a cut behind the last
    # character leaves a text of the chunk's length flat
    assert (flat > 0) == (kind in ("alpha", "eq", "cut"))


def test_one_shot_candidates():
    """The candidate test: the unbroken text's length and not the encoder's, of
    more than 54 bytes: up to there the one-pass decode takes the unbroken text."""
    for size in range(0, 400):
        d = W.chunk_bytes(size)
        flat, enc = F.text(d), W.xmlrpc_text(d)
        assert F.is_candidate(len(flat), size) == (size > 54) == (not W.is_encoder_layout(flat)), size
        assert (flat != enc) == (size >= 54)
        assert not F.is_candidate(len(enc), size) or size <= 54
        assert F.is_flat(flat) == (size > 0) and base64.b64decode(flat, validate=True) == W.decode(flat) == d
        if size > 54:
            assert F.decoded_flat(flat, size) and not W.is_encoder_layout(flat)
    lib = _capi.load()
    for size in (0, 1, 54, 55, 56, 57, 864, 262144):
        assert lib.lbf_b64_put_length(size) == W.b64_len(size)


# ------------------------------------------------------------ 2. the encoder's layout
@pytest.mark.parametrize("size", W.PERIOD_SIZES)
def test_encoder_layout_is_left_to_the_line_path(size):
    """Every two-way cut of the 16-line texts: behind the line model's prefix
    the flat path takes at most one line, and what it takes is the general
    rule's."""
    t = W.xmlrpc_text(W.chunk_bytes(size))
    most = 0
    for a in range(len(t) + 1):
        state = M.init()
        for piece in (t[:a], t[a:]):
            n1, _, after = L.take(state, piece)
            n, _ = check_rest(after, piece[n1:], (size, a))
            assert n <= 72, (size, a, n)
            assert F.most_behind_lines(n1, piece) <= 72
            most = max(most, n)
            state, _ = M.update(state, piece)
    assert most <= 8  # the line model leaves less than two groups and a separator


def test_bound_behind_the_line_path():
    """most_behind_lines: no flat prefix that starts at or before the line
    model's stop is longer."""
    rng = np.random.default_rng(5)
    for _ in range(300):
        t = bytearray(W._alpha_stream(int(rng.integers(1, 200)), int(rng.integers(0, 1 << 30))))
        for p in rng.integers(0, len(t), int(rng.integers(0, 5))):
            t[int(p)] = (ord(" "), ord("="), ord("*"))[int(p) % 3]
        t = bytes(t)
        stop = int(rng.integers(0, len(t) + 1))
        bound = F.most_behind_lines(stop, t)
        for a in range(0, stop + 1):
            assert F.take(M.init(), t[a:])[0] <= bound, (t, stop, a)


# ------------------------------------------------------------ 3. the entry points
def test_symbols_exported():
    import bitflood_amd
    from bitflood_amd import hashing
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in ("lbf_set_b64_flat", "lbf_ctx_b64_flat_stats"):
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s
    assert {"set_b64_flat"} <= set(hashing.__all__) and callable(bitflood_amd.set_b64_flat)
    assert hasattr(hashing.ChunkHasher, "b64_flat_stats")
    # the switch needs no GPU: it returns the previous value
    first = hashing.set_b64_flat(False)
    assert hashing.set_b64_flat(True) is False
    assert hashing.set_b64_flat(first) is True
    header = open(_capi.HEADER_PATH).read()
    assert "sub-count of lbf_ctx_b64_stats' general_chunks" in header
    assert "sub-count of lbf_ctx_b64_update_stats' scan_chars" in header


def test_flat_kernels_are_in_the_source_list():
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert "b64_flat.hip" in srcs and "b64_update_lines.hip" in srcs and "b64_update.hip" in srcs


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_flat_kernels_resources(tmp_path):
    """Two kernels, nothing in scratch, nothing spilled, at most 64 VGPRs (eight
    waves per SIMD), and LDS for eight workgroups to a CU (two staged tiles of
    text, the table, the flags)."""
    src = os.path.join(CSRC, "b64_flat.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / "f.o"),
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks}
    assert len(kernels) == 2, sorted(kernels)
    assert sum("b64_flat_decode_kernel" in k for k in kernels) == 1, sorted(kernels)
    assert sum("b64_update_flat_kernel" in k for k in kernels) == 1, sorted(kernels)
    for rem in kernels.values():
        assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
        assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
        assert re.search(r"Dynamic Stack: False", rem), rem
        assert int(re.search(r" VGPRs: (\d+)", rem).group(1)) <= 64, rem
        lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", rem).group(1))
        assert 2 * F.TILE_TEXT <= lds <= 20480, lds
    text = open(src).read()
    assert "asm" not in text.replace("__launch_bounds__", "")  # no inline assembly, and only barriers synchronise
    assert "while (" not in text and "__syncthreads()" in text
    # the tile the model restates
    assert re.search(r"kTileBytes = (\d+)", text).group(1) == str(F.TILE_BYTES)

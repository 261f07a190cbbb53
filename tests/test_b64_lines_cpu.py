"""The line path of the piecewise base64 decode, the parts that need no GPU:
its rule (tests/wire_line_model.py) against the general rule
(tests/wire_piece_model.update, pinned to xmlrpc++'s recorded answers) on every
cut of the 16-line texts and next to every damage, the new entry points, and
the line kernel's resource usage on gfx950."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from bitflood_amd import _capi
from tests import wire_layouts as W
from tests import wire_line_model as L
from tests import wire_piece_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")


def conforms(state, prefix: bytes) -> bool:
    """Every character of `prefix` stands where the layout puts one of its
    kind, counted from the state's column -- worked out per character, not by
    walking groups as the model does.  A leading separator at column 0 is let
    through; '=' conforms nowhere."""
    decoded, carry, _ = state
    col = (4 * decoded // 3 + len(carry)) % 72
    v = M.TABLE[np.frombuffer(prefix, dtype=np.uint8)]
    if col == 0 and v.size and v[0] == M.SKIP:
        v = v[1:]
    place = (col + np.arange(v.size)) % 73
    return bool(np.where(place == 72, v == M.SKIP, v < M.EQ).all())


def check_piece(state, piece: bytes, what):
    """The model's prefix of `piece` against the general rule; returns its length."""
    n, body, after = L.take(state, piece)
    assert 0 <= n <= len(piece), what
    want_state, want = M.update(state, piece[:n])
    assert body == want and after == want_state, (what, n)
    assert conforms(state, piece[:n]) and b"=" not in piece[:n], (what, n)
    if n == 0:
        assert after == state, what  # nothing taken: the carry, if any, stays for the general rule
    else:
        assert len(after[1]) == 0 and not after[2] and after[0] % 3 == 0, what
    return n


@pytest.mark.parametrize("size", W.PERIOD_SIZES)
def test_prefix_is_the_general_rule_at_every_cut(size):
    """Both pieces of every two-way cut: the prefix decodes by places to what
    the general rule gives, leaves nothing carried, and leaves at most a
    separator, three characters of an unfinished group or the '=' group."""
    t = W.xmlrpc_text(W.chunk_bytes(size))
    lead = set()
    for a in range(len(t) + 1):
        n1 = check_piece(M.init(), t[:a], (size, a, 1))
        assert a - n1 <= 8, (size, a, n1)
        state, _ = M.update(M.init(), t[:a])
        if state[2]:
            assert L.take(state, t[a:])[0] == 0  # the data has ended: nothing for the line path
            continue
        n2 = check_piece(state, t[a:], (size, a, 2))
        assert len(t) - a - n2 <= 8, (size, a, n2)
        if a < len(t) and (4 * state[0] // 3 + len(state[1])) % 72 == 0:
            lead.add((state[0] > 0, t[a:a + 1] == b" "))
    # column 0 with and without the separator in front, at the text's start and further in
    assert lead == {(False, False), (True, False), (True, True)}


def test_leading_separator_at_the_start_of_a_chain():
    """S = 0 and a separator in front: taken, as the general rule skips it."""
    t = W.xmlrpc_text(W.chunk_bytes(300))
    n = check_piece(M.init(), b" " + t, "sep first")
    assert n == 1 + len(t)
    assert check_piece(M.init(), b"=" + t, "eq first") == 0
    assert check_piece(M.init(), b"  " + t, "two separators") == 1


@pytest.mark.parametrize("kind", W.KINDS)
def test_prefix_next_to_damage(kind):
    """period_corpus(kind), each text cut two characters before its damage: the
    second piece's prefix holds no character that breaks the layout, and by
    places it decodes to what the general rule gives."""
    corpus = W.period_corpus(kind)
    places = []
    for size in W.PERIOD_SIZES:
        t = W.xmlrpc_text(W.chunk_bytes(size))
        places += [None] + list(W.positions(len(t), kind))
    assert len(places) == len(corpus)
    short = 0
    for t, p in zip(corpus.texts, places):
        a = len(t) // 2 if p is None else max(p - 2, 0)
        state, _ = M.update(M.init(), t[:a])
        if state[2]:
            continue
        n = check_piece(state, t[a:], (kind, p))
        short += n < len(t) - a - 8
    assert short > 0 or kind == "cut"  # damage stops the prefix somewhere (alpha: at a separator); a cut text just ends


def test_symbols_exported():
    from bitflood_amd import hashing
    lib = _capi.load()
    syms = _capi.header_symbols()
    for s in ("lbf_set_b64_lines", "lbf_ctx_b64_update_stats"):
        assert s in syms and s in _capi._SIGS and hasattr(lib, s), s
    assert {"set_b64_lines"} <= set(hashing.__all__)
    assert hasattr(hashing.ChunkHasher, "b64_update_stats") and callable(hashing.set_b64_lines)
    # the switch needs no GPU: it returns the previous value
    first = hashing.set_b64_lines(False)
    assert hashing.set_b64_lines(True) is False
    assert hashing.set_b64_lines(first) is True
    header = open(_capi.HEADER_PATH).read()
    assert "four enqueues" in header and "three enqueues, no host" not in header


def test_line_kernel_is_in_the_source_list():
    srcs = subprocess.run(["make", "-s", "-C", CSRC, "sources"], capture_output=True, text=True,
                          check=True).stdout.split()
    assert "b64_update_lines.hip" in srcs and "b64_update.hip" in srcs


@pytest.mark.skipif(not (os.path.exists(HIPCC) or shutil.which("hipcc")), reason="no hipcc")
def test_line_kernel_resources(tmp_path):
    """One kernel, nothing in scratch, nothing spilled, and LDS for eight
    workgroups to a CU (two staged tiles of text, the table, the flags)."""
    src = os.path.join(CSRC, "b64_update_lines.hip")
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-I" + os.path.join(ROOT, "include"),
                        "-I" + CSRC, "--offload-device-only", "-c", "-o", str(tmp_path / "l.o"),
                        "-Rpass-analysis=kernel-resource-usage", src], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    blocks = re.split(r"remark: Function Name: ", r.stderr)[1:]
    kernels = {b.split()[0]: b for b in blocks}
    assert len(kernels) == 1 and "b64_update_lines_kernel" in next(iter(kernels)), sorted(kernels)
    rem = next(iter(kernels.values()))
    assert re.search(r"ScratchSize \[bytes/lane\]: 0\b", rem), rem
    assert re.search(r"VGPRs Spill: 0\b", rem) and re.search(r"SGPRs Spill: 0\b", rem), rem
    assert re.search(r"Dynamic Stack: False", rem), rem
    lds = int(re.search(r"LDS Size \[bytes/block\]: (\d+)", rem).group(1))
    assert 2 * 5256 <= lds <= 20480, lds
    text = open(src).read()
    assert "asm" not in text.replace("__launch_bounds__", "")  # no inline assembly, and only barriers synchronise
    assert "while (" not in text

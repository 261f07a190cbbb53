"""tests/wire_layouts.py: its reference is the reference's, and its corpora
reach what tests/test_gpu_wire.py relies on them to reach.  No GPU.

The decode rules (junk skipped, '=' ends the data, a group cut short is
dropped) are held against outputs recorded from xmlrpc++ 0.7's own decoder
and encoder (tests/golden/xmlrpc07_base64_get.json, written by
tests/golden/make_xmlrpc_b64_fixture.py): the character-by-character
restatement `b64get`, the vectorised `decode` the GPU tests use, and the
host's C++ restatement PeerWire::Base64Get / Base64Put (tests/c/b64get_lines)
all give the recorded bytes.  The geometry the corpora are built around is
read back from the kernels' sources.
"""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import wire_layouts as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bitflood_amd", "csrc")
LINES_EXE = os.path.join(ROOT, "tests", "c", "build", "b64get_lines")


@pytest.fixture(scope="module")
def recorded(golden):
    return golden("xmlrpc07_base64_get.json")


def _lines(mode, items):
    if not os.path.exists(LINES_EXE):
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "tests", "c")])
    text = "".join((b.hex() or "-") + "\n" for b in items)
    out = subprocess.run([LINES_EXE, mode], input=text, capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    got = [bytes.fromhex("" if line == "-" else line) for line in out.stdout.splitlines()]
    assert len(got) == len(items)
    return got


# ------------------------------------------------------------------ geometry
def test_geometry_constants_are_the_kernels():
    hpp = open(os.path.join(CSRC, "kern_b64.hpp")).read()
    hip = open(os.path.join(CSRC, "sha1_kernels.hip")).read()

    def define(name):
        return int(re.search(rf"^#define {name} (\d+)\b", hpp, re.M).group(1))

    assert define("LBF_B64_DEC_LINES") == W.DEC_LINES
    assert define("LBF_B64_DEC_TILES_PER_GROUP") == W.DEC_TILES_PER_GROUP
    assert define("LBF_B64_ENC_LINES") == W.ENC_LINES
    assert define("LBF_B64_ENC_TILES_PER_GROUP") == W.ENC_TILES_PER_GROUP
    threads = int(re.search(r"constexpr int kB64Threads = (\d+);", hpp).group(1))
    # pass 1 takes 16 characters per lane and trip, pass 2 four groups
    assert "tile += kB64Threads * 16" in hpp and "g4 += kB64Threads * 4" in hpp
    assert threads * 16 == W.SCAN_CHARS and threads * 4 == W.SCAN_GROUPS
    assert "kDecText = kDecLines * 73, kDecBytes = kDecLines * 54" in hpp
    assert "kB64TileText = kB64TileLines * 73;" in hpp and "kB64TileBytes = kB64TileLines * 54;" in hpp
    launch = hip[hip.index("static int b64_tiled_launch"):]
    assert int(re.search(r"constexpr uint32_t kPer = (\d+);", launch).group(1)) == W.CHUNKS_PER_LAUNCH
    assert (W.DEC_TEXT, W.DEC_BYTES, W.ENC_TEXT, W.ENC_BYTES) == (5256, 3888, 8176, 6048)


# -------------------------------------------------- the reference's own codec
def test_decoders_give_what_xmlrpc_recorded(recorded):
    rows = recorded["get"]
    assert len(rows) > 300
    texts = [bytes.fromhex(r[0]) for r in rows]
    want = [bytes.fromhex(r[1]) for r in rows]
    # every kind at every position of the short texts, and around the separator of the long one
    assert {len(t) for t in texts} >= set(range(0, 10)) | {76, 77, 78}
    assert any(w for w in want) and any(not w and t for t, w in zip(texts, want))
    for t, w in zip(texts, want):
        assert W.b64get(t) == w, t
        assert W.decode(t) == w, t
    assert _lines("get", texts) == want


def test_encoders_give_what_xmlrpc_recorded(recorded):
    rows = recorded["put"]
    chunks = [bytes.fromhex(r[0]) for r in rows]
    texts = [bytes.fromhex(r[1]) for r in rows]
    assert [len(c) for c in chunks] == list(range(9)) + list(range(53, 58)) + [107, 108, 109]
    for c, t in zip(chunks, texts):
        assert W.xmlrpc_text(c) == t.replace(b"\n", b" "), len(c)
        assert W.decode(t) == c
    assert _lines("put", chunks) == texts  # Base64Put writes the newlines themselves


def _random_damage_corpus(n, seed):
    rng = np.random.default_rng(seed)
    junk = [c for c in range(256) if W._DEC[c] == W.SKIP]
    texts = []
    for case in range(n):
        size = int(rng.integers(0, 3000 if case % 50 == 0 else 400))
        t = W.xmlrpc_text(rng.integers(0, 256, size, dtype=np.uint8).tobytes())
        for _ in range(int(rng.integers(0, 4))):
            kind = W.KINDS[int(rng.integers(0, len(W.KINDS)))]
            ps = W.positions(len(t), kind)
            if len(ps):
                t = W.damage(t, kind, int(rng.integers(0, len(ps))))
        if case % 3 == 0 and t:
            b = bytearray(t)
            for _ in range(int(rng.integers(1, 20))):
                b.insert(int(rng.integers(0, len(b) + 1)), int(rng.choice(junk)))
            t = bytes(b)
        texts.append(t)
    return texts


def test_vectorised_decode_is_b64get():
    texts = _random_damage_corpus(2000, seed=17)
    assert sum(b"=" in t[:-2] for t in texts) > 200 and sum(len(t) % 4 != 0 for t in texts) > 500
    for t in texts:
        assert W.decode(t) == W.b64get(t), t


def test_encoder_texts_have_the_encoder_layout():
    for n in range(401):
        t = W.xmlrpc_text(W.chunk_bytes(n))
        assert W.is_encoder_layout(t), n
        if n:
            assert len(t) % 73 == 72 or len(t) % 73 % 4 == 0
    t = W.xmlrpc_text(W.chunk_bytes(110))  # a line, a separator, 18 groups, a separator, "xxx="
    assert len(t) == 2 * 73 + 4 and t[-1:] == b"="
    sep, inside = 72, 30
    assert W.is_encoder_layout(W.damage(t, "junk", sep))
    assert not W.is_encoder_layout(W.damage(t, "alpha", sep))
    assert not W.is_encoder_layout(W.damage(t, "eq", sep))
    assert not W.is_encoder_layout(W.damage(t, "junk", inside))
    assert not W.is_encoder_layout(W.damage(t, "eq", inside))
    assert W.is_encoder_layout(W.damage(t, "alpha", inside))
    assert not W.is_encoder_layout(W.damage(t, "drop", inside))
    assert not W.is_encoder_layout(W.damage(t, "ins_alpha", inside))
    assert W.is_encoder_layout(W.damage(t, "cut", 73)) and W.is_encoder_layout(W.damage(t, "cut", 72))
    assert W.is_encoder_layout(W.damage(t, "cut", 8)) and not W.is_encoder_layout(W.damage(t, "cut", 74))
    assert W.is_encoder_layout(t[:-2] + b"==") and not W.is_encoder_layout(t[:-2] + b"=A")
    assert not W.is_encoder_layout(t[:-3] + b"===")


def test_filler_text_is_the_encoders():
    for n in list(range(0, 120)) + [3888, 3889, 3890, 20000]:
        assert W.filler_text(n) == W.xmlrpc_text(b"\xEE" * n), n
        assert W.b64_len(n) == len(W.filler_text(n))


# ------------------------------------------------- what the GPU corpora reach
def test_period_corpus_meets_every_block_phase_and_lane_byte_at_every_column():
    """Test 1: 16 lines are a period of the 73-character lines against the
    one-pass decode's 16-byte blocks (whose bytes start at phase b0 % 3 of a
    group) and against the general decode's 16-character lanes."""
    for n in W.PERIOD_SIZES:
        t = W.xmlrpc_text(W.chunk_bytes(n))
        assert len(t) // 73 == 16 and len(t) < W.DEC_TEXT and len(t) < W.SCAN_CHARS
        ps = list(W.positions(len(t), "junk"))
        assert ps == list(range(len(t)))
        block_col = {(u % 3, p % 73) for p in ps for u in W.one_pass_blocks(p)}  # b0 = 16u, so b0 % 3 = u % 3
        assert block_col >= {(ph, col) for ph in range(3) for col in range(73)}
        lane_col = {(p % 16, p % 73) for p in ps}
        assert lane_col == {(b, col) for b in range(16) for col in range(73)}
    for kind in W.KINDS:
        c = W.period_corpus(kind)
        want = sum(len(W.positions(len(W.xmlrpc_text(W.chunk_bytes(n))), kind)) + 1 for n in W.PERIOD_SIZES)
        assert len(c) == want and 3500 < len(c) < 3530
        assert sum(t == W.xmlrpc_text(d) for t, d in zip(c.texts, c.chunks)) >= 3
    one, general = W.period_corpus("drop").layout_counts()
    # a dropped character leaves the layout, except the separator that ends the 864-byte chunk's text
    assert one == 3 + 1
    one, general = W.period_corpus("alpha").layout_counts()
    # an alphabet character in a separator's place, and "xx=Q" for the 865-byte chunk's "xx=="
    assert general == 3 * 16 + 1


def test_one_pass_blocks_are_the_kernels_windows():
    """one_pass_blocks restates b64_decode_block's window: block u holds bytes
    [16u, +16) = groups g0 .. g0 + 5, g0 = 16u // 3."""
    for pos in range(0, 3 * 73):
        line, col = divmod(pos, 73)
        for u in W.one_pass_blocks(pos):
            g0 = 16 * u // 3
            g = 18 * line + (col // 4 if col < 72 else 17)
            assert g0 <= g <= g0 + 5
            if col < 72:
                assert 16 * u < 3 * g + 3 and 3 * g < 16 * u + 16
        assert W.one_pass_blocks(pos)


def test_edge_corpus_lies_on_both_sides_of_every_edge():
    """Test 2: five decode tiles and a part, two workgroups, seven scan trips."""
    for n in W.EDGE_SIZES:
        tl = len(W.xmlrpc_text(W.chunk_bytes(n)))
        assert -(-tl // W.DEC_TEXT) == 6 and tl % W.DEC_TEXT and -(-tl // W.SCAN_CHARS) == 7
        assert -(-6 // W.DEC_TILES_PER_GROUP) == 2
        assert -(-(tl // 73 * 18) // W.SCAN_GROUPS) == 7
        ps = set(W.edge_positions(tl))
        for tile in (1, W.DEC_TILES_PER_GROUP, 5):
            edge = tile * W.DEC_TEXT
            assert set(range(edge - 73, edge + 73)) <= ps
        for k in (1, 2, 6):
            assert set(range(4096 * k - 17, 4096 * k + 18)) <= ps
        assert set(range(tl - 80, tl)) <= ps
        assert max(ps) == tl - 1 and 600 < len(ps) < 640
    assert W.chunk_bytes(20674) != W.chunk_bytes(20675)[:-1]
    for kind in ("junk", "ins_eq", "cut"):
        c = W.edge_corpus(kind)
        assert 1200 < len(c) < 1290
        assert any(d.endswith(" undamaged") for d in c.desc)


def test_disagreeing_lengths_cross_whole_tiles_and_workgroups_both_ways():
    """Test 3: the tiles a chunk's workgroups cover are max(text tiles, slot
    tiles); the pairs have the slot run whole tiles and a whole workgroup past
    the text, and the text past the slot."""
    D, G = W.DEC_BYTES, W.DEC_BYTES * W.DEC_TILES_PER_GROUP
    assert (D, G) == (3888, 15552)
    tiles = lambda n: -(-n // D)  # noqa: E731  (tiles of L decoded bytes = tiles of its text)
    groups = lambda n: -(-tiles(n) // W.DEC_TILES_PER_GROUP)  # noqa: E731
    pairs = W.DISAGREE_PAIRS
    assert len(pairs) == 15
    assert any(tiles(C) - tiles(L) >= W.DEC_TILES_PER_GROUP and groups(C) > max(groups(L), 1) for L, C in pairs)
    assert any(tiles(L) - tiles(C) >= W.DEC_TILES_PER_GROUP and groups(L) > max(groups(C), 1) for L, C in pairs)
    assert any(tiles(C) - tiles(L) == 1 for L, C in pairs) and any(tiles(L) - tiles(C) == 1 for L, C in pairs)
    assert any(C == 0 for _, C in pairs) and any(L == 0 for L, _ in pairs)
    for L in (40, D - 1, D, D + 1, G + D):
        tl = len(W.xmlrpc_text(bytes(L)))
        assert tl <= tiles(L) * W.DEC_TEXT and tiles(L) == -(-tl // W.DEC_TEXT)
    c = W.disagree_corpus()
    assert len(c) == 15 * 8
    seen = set()
    for t, d, cap, tp, sp, what in zip(c.texts, c.chunks, c.caps, c.tphase, c.sphase, c.desc):
        general = " general " in what
        assert W.is_encoder_layout(t) is not general, what
        L = len(W.decode(t))
        assert len(d) == cap
        seen.add((L, cap, general, sp, tp))
    assert seen == {(L, C, g, sp, tp) for L, C in pairs for g in (False, True) for sp in (0, 5) for tp in (0, 3)}
    verdicts = [v for _, _, v in c.expected()]
    assert not any(verdicts)  # no pair has L == C
    assert c.layout_counts() == (60, 60)


def test_scan_families_meet_every_phase_and_are_what_they_are_called():
    fam = W.scan_families()
    assert set(fam) == {"woven", "junk-run", "first-eq", "two-eq", "length", "groups"}
    valid = lambda t: W._DEC[np.frombuffer(t, np.uint8)] != W.SKIP  # noqa: E731
    stream = lambda t: W._DEC[np.frombuffer(t, np.uint8)][valid(t)]  # noqa: E731
    for name, texts in fam.items():
        for t, what in texts:
            assert not W.is_encoder_layout(t), (name, what)
    # woven: in every trip the lanes hold every count 0..16
    for t, _ in fam["woven"]:
        v = valid(t + b"\0" * (-len(t) % 16)).reshape(-1, 16).sum(axis=1)
        assert len(t) > 2 * W.SCAN_CHARS
        for trip in range(len(t) // W.SCAN_CHARS):
            assert set(v[256 * trip:256 * trip + 256]) == set(range(17))
    # junk-run: a whole trip without one valid character, at the start, inside and at the end
    where = set()
    for t, _ in fam["junk-run"]:
        v = valid(t)
        trips = -(-len(t) // W.SCAN_CHARS)
        empty = [k for k in range(trips) if not v[4096 * k:4096 * k + 4096].any()]
        assert empty and v.any()
        where |= {"first" if 0 in empty else "", "last" if trips - 1 in empty else "",
                  "inside" if any(0 < k < trips - 1 for k in empty) else ""}
    assert where >= {"first", "last", "inside"}
    # first-eq: stream index = text index, first '=' at 4096k + j, valid characters and '=' behind it
    qs = []
    for t, _ in fam["first-eq"]:
        s = stream(t)
        assert s.size == len(t)
        eq = np.flatnonzero(s == W.EQ)
        qs.append(int(eq[0]))
        assert eq.size >= 3 and (s[eq[0]:] < W.EQ).sum() >= 5000 and eq[-1] // 4096 > eq[0] // 4096
    assert sorted(qs) == [4096 * k + j for k in (1, 2) for j in range(-5, 6)]
    for k in (1, 2):
        assert {q % 4 for q in qs if q < 4096 * k and q > 4096 * k - 6} == {0, 1, 2, 3}
        assert {q % 4 for q in qs if 4096 * k <= q < 4096 * k + 6} == {0, 1, 2, 3}
    # two-eq: both in one trip, in different waves of 64 lanes x 16 characters
    for t, _ in fam["two-eq"]:
        eq = np.flatnonzero(np.frombuffer(t, np.uint8) == ord("="))
        assert eq.size == 2 and eq[0] // 4096 == eq[1] // 4096 and eq[0] % 4096 // 1024 != eq[1] % 4096 // 1024
    assert {t.index(b"=") // 4096 for t, _ in fam["two-eq"]} == {0, 1, 2}
    assert sorted(len(t) for t, _ in fam["length"]) == sorted(
        4096 * k + d for k in (1, 2) for d in (-16, -15, -1, 0, 1, 15, 16, 17))
    got = sorted((stream(t).size // 4, stream(t).size % 4) for t, _ in fam["groups"])
    assert [g for g, _ in got] == sorted(1024 * k + d for k in (1, 2, 3) for d in range(-1, 6))
    assert {r for _, r in got} == {0, 1, 2, 3}
    # the rotation
    c = W.scan_corpus()
    assert len(c) == sum(len(v) for v in fam.values())
    for name in fam:
        rows = [i for i, d in enumerate(c.desc) if f" {name}: " in d]
        assert len(rows) == len(fam[name])
        assert {c.tphase[i] for i in rows} == {0, 1, 2, 3}, name
        assert {c.sphase[i] for i in rows} == {0, 1, 2, 3}, name
        assert {c.caps[i] - len(c.chunks[i]) for i in rows} >= {0, -1, -5, 9}, name
    assert c.layout_counts() == (0, len(c))


def test_slices_corpus_passes_one_launch_slice():
    c = W.slices_corpus()
    assert len(c) == W.CHUNKS_PER_LAUNCH + 300
    tail = range(W.CHUNKS_PER_LAUNCH, len(c))
    assert sum(not c.digest_ok[i] for i in tail) >= 27 and sum(" junk " in c.desc[i] for i in tail) >= 42
    assert {len(d) for d in c.chunks} == set(range(61))
    one, general = c.layout_counts()
    assert general > 9000 and one > 56000
    assert sum(not ok for ok in c.digest_ok) == -(-len(c) // 11)
    # the chunks past the slice differ from the ones a wrong first-chunk index would read
    assert [c.texts[i] for i in tail] != [c.texts[i - W.CHUNKS_PER_LAUNCH] for i in tail]


def test_encode_cases_meet_every_source_phase_at_the_tile_edges():
    cases = W.encode_cases()
    sizes = {s for s, _, _ in cases}
    assert sizes == {6048 * k + d for k in (1, 2, 3, 4) for d in range(-3, 4)} | {
        54 * j + d for j in (0, 1, 17, 18, 112) for d in (0, 1, 2)}
    for k in (1, 2):
        for d in range(-3, 4):
            assert {p for s, p, _ in cases if s == 6048 * k + d} == set(range(16)), (k, d)
    rest = [(s, p, t) for s, p, t in cases if not 6048 - 3 <= s <= 6048 + 3 and not 12096 - 3 <= s <= 12096 + 3]
    assert len(rest) == 14 + 12 and len({p for _, p, _ in rest}) >= 12  # 54 * 112 + {0, 1, 2} are tile-edge sizes too
    assert {t for _, _, t in cases} == {0, 1, 8, 15} == {t for _, _, t in rest}
    # two tiles to a workgroup: sizes past 12,096 bytes take a second workgroup
    assert W.ENC_BYTES * W.ENC_TILES_PER_GROUP == 12096 and max(sizes) > 2 * 12096 - 4
    assert len(cases) < 300

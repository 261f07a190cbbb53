"""Texts for the wire (base64) kernels of bitflood_amd/csrc/kern_b64.hpp, and
the reference they are compared with.  No GPU, no pytest.

The receiver's decode follows xmlrpc++ 0.7's decoder (base64.h:215-330), the
sender's encode its encoder (base64.h:154-210).  `b64get` restates the decoder
character by character; `decode` is the same rule vectorised (fast enough for
corpora of thousands of texts); tests/test_wire_layouts.py pins both, and
bitflood_amd/host/PeerWire.cpp's restatement, to outputs recorded from the
reference's own decoder (tests/golden/xmlrpc07_base64_get.json).

The corpus builders place damage by the kernels' structure rather than at
random: every character position of a period of the line/block/lane grids,
both sides of every tile, workgroup and scan-trip edge, slots and texts whose
lengths disagree by whole tiles, and batches past one launch slice.
tests/test_wire_layouts.py proves what each corpus reaches;
tests/test_gpu_wire.py runs them.
"""
import base64
import functools

import numpy as np

EQ, SKIP = 64, 255
ALPHABET = b"ABCDEFGHIJKLMNOPQRSTUVWXYZabcdefghijklmnopqrstuvwxyz0123456789+/"
_DEC = np.full(256, SKIP, dtype=np.int16)
for _i, _c in enumerate(ALPHABET):
    _DEC[_c] = _i
_DEC[ord("=")] = EQ

# ---- the kernels' geometry, restated (tests/test_wire_layouts.py reads the
# ---- sources and fails if these drift)
LINE_CHARS, LINE_BYTES, LINE_GROUPS = 73, 54, 18
DEC_LINES, DEC_TILES_PER_GROUP = 72, 4       # the one-pass decode's tile and workgroup
ENC_LINES, ENC_TILES_PER_GROUP = 112, 2      # the encode's
SCAN_CHARS, SCAN_GROUPS = 4096, 1024         # the general decode's pass-1 and pass-2 trips
CHUNKS_PER_LAUNCH = 65535                    # grid.y of one tiled launch
DEC_TEXT, DEC_BYTES = DEC_LINES * LINE_CHARS, DEC_LINES * LINE_BYTES    # 5,256 / 3,888
ENC_TEXT, ENC_BYTES = ENC_LINES * LINE_CHARS, ENC_LINES * LINE_BYTES    # 8,176 / 6,048

JUNK = (0x00, ord("\n"), ord("*"), ord("-"), 0x7F, 0x80, 0xFF)
KINDS = ("junk", "eq", "alpha", "drop", "ins_junk", "ins_eq", "ins_alpha", "cut")


# ---------------------------------------------------------------- the reference
def b64get(text: bytes) -> bytes:
    """xmlrpc++ 0.7 base64 decode (base64.h:215-330): skip characters outside
    the alphabet; take the rest four at a time; a group holding '=' ends the
    data ("xx==" one byte, "xxx=" two); an incomplete last group is dropped."""
    v = _DEC[np.frombuffer(text, dtype=np.uint8)]
    s = v[v != SKIP]
    out = bytearray()
    i = 0
    while True:
        if i >= len(s) or s[i] == EQ:
            return bytes(out)
        if i + 1 >= len(s) or s[i + 1] == EQ:
            return bytes(out)
        c0, c1 = int(s[i]), int(s[i + 1])
        if i + 2 >= len(s):
            return bytes(out)
        c2 = int(s[i + 2])
        if c2 == EQ:
            out.append(((c0 << 2) | (c1 >> 4)) & 255)
            return bytes(out)
        if i + 3 >= len(s):
            return bytes(out)
        c3 = int(s[i + 3])
        if c3 == EQ:
            out += bytes([((c0 << 2) | (c1 >> 4)) & 255, ((c1 << 4) | (c2 >> 2)) & 255])
            return bytes(out)
        out += bytes([((c0 << 2) | (c1 >> 4)) & 255, ((c1 << 4) | (c2 >> 2)) & 255, ((c2 << 6) | c3) & 255])
        i += 4


def xmlrpc_text(data: bytes) -> bytes:
    """The payload text of a SendChunk frame: base64 with a newline after
    every 18th complete group (base64.h:197-205), CR/LF framed as spaces."""
    s = base64.b64encode(data)
    full = len(data) // 3
    if full < 18:  # no line is complete: no separator
        return s
    parts = []
    for g in range(len(s) // 4):
        parts.append(s[4 * g:4 * g + 4])
        if g < full and g % 18 == 17:
            parts.append(b" ")
    return b"".join(parts)


def decode(text: bytes) -> bytes:
    """b64get's rules without its loop: S = the characters of the alphabet and
    '=' in order, q = the index of the first '=' in S (len(S) if none); the
    3 * (q // 4) bytes of the complete groups, then one byte when q % 4 == 2
    and S[q] is '=', two when q % 4 == 3."""
    v = _DEC[np.frombuffer(text, dtype=np.uint8)]
    s = v[v != SKIP].astype(np.uint32)
    eq = np.flatnonzero(s == EQ)
    q = int(eq[0]) if eq.size else s.size
    g = q // 4
    x = s[:4 * g].reshape(g, 4)
    w = (x[:, 0] << 18) | (x[:, 1] << 12) | (x[:, 2] << 6) | x[:, 3]
    out = np.empty((g, 3), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = w >> 16, (w >> 8) & 255, w & 255
    tail = b""
    if q < s.size and q % 4 >= 2:
        c = [int(k) for k in s[4 * g:q]]
        tail = bytes([((c[0] << 2) | (c[1] >> 4)) & 255])
        if q % 4 == 3:
            tail += bytes([((c[1] << 4) | (c[2] >> 2)) & 255])
    return out.tobytes() + tail


def is_encoder_layout(text: bytes) -> bool:
    """The one-pass decode's contract (kern_b64.hpp, "One pass for text laid
    out as the encoder writes it"): the length is 73q + 4r or 73q + 72; group g
    sits at 4g + g // 18, all in the alphabet, except that the last may be
    "xx==" or "xxx="; every separator place (73l + 72) holds a character that is
    neither in the alphabet nor '='.  Those places are all of the text, so
    nothing else is present."""
    n = len(text)
    q, rem = divmod(n, LINE_CHARS)
    if rem == 72:
        groups = 18 * q + 18
    elif rem % 4 == 0:
        groups = 18 * q + rem // 4
    else:
        return False
    if groups == 0:
        return True
    c = _DEC[np.frombuffer(text, dtype=np.uint8)]
    if n > 72:
        sep = np.arange(72, n, LINE_CHARS)
        if (c[sep] != SKIP).any():
            return False
        body = np.ones(n, dtype=bool)
        body[sep] = False
        c = c[body]  # 4 * groups characters
    assert c.size == 4 * groups
    if (c[:-2] >= EQ).any():  # everything up to the last group's first two characters
        return False
    c2, c3 = int(c[-2]), int(c[-1])
    return (c2 < EQ and c3 < EQ) or (c2 < EQ and c3 == EQ) or (c2 == EQ and c3 == EQ)


def damage(text: bytes, kind: str, pos: int) -> bytes:
    """One damaged copy of `text`.  junk / eq / alpha replace character `pos`
    (junk cycles through JUNK by position; alpha puts another alphabet
    character, 'Q' where the text holds none, as at a separator); drop removes
    it; ins_* insert in front of it (pos == len(text) appends); cut keeps
    `pos` characters."""
    t = bytearray(text)
    if kind == "cut":
        return bytes(t[:pos])
    if kind.startswith("ins_"):
        c = {"ins_junk": JUNK[pos % len(JUNK)], "ins_eq": ord("="), "ins_alpha": ALPHABET[pos % 64]}[kind]
        t.insert(pos, c)
        return bytes(t)
    if kind == "drop":
        del t[pos]
    elif kind == "junk":
        t[pos] = JUNK[pos % len(JUNK)]
    elif kind == "eq":
        t[pos] = ord("=")
    elif kind == "alpha":
        t[pos] = ord("Q") if _DEC[t[pos]] >= EQ else (ord("A") if t[pos] != ord("A") else ord("B"))
    else:
        raise ValueError(kind)
    return bytes(t)


def positions(text_len: int, kind: str):
    """The positions `damage` takes for a text of that length."""
    return range(text_len + 1) if kind == "cut" or kind.startswith("ins_") else range(text_len)


def b64_len(size: int) -> int:
    """The length of xmlrpc_text(size bytes)."""
    return 4 * (size // 3) + (4 if size % 3 else 0) + size // 3 // 18


def filler_text(nbytes: int) -> bytes:
    """xmlrpc_text(b'\\xEE' * nbytes), built from its period (three 0xEE bytes
    are "7u7u") so that a text of tens of megabytes costs nothing."""
    full, rest = divmod(nbytes, 3)
    lines, r = divmod(full, 18)
    return (b"7u7u" * 18 + b" ") * lines + b"7u7u" * r + (b"", b"7g==", b"7u4=")[rest]


# ------------------------------------------------------------- where a place lies
def one_pass_blocks(pos: int):
    """The one-pass decode's blocks (16 output bytes each; block u of the
    chunk is lane u % 243 of tile u // 243) that read text character `pos`: the
    blocks whose bytes its group holds, or for a separator the blocks whose
    six-group window holds the line's last group."""
    line, col = divmod(pos, LINE_CHARS)
    g = 18 * line + (col // 4 if col < 72 else 17)
    if col < 72:
        return sorted({(3 * g) // 16, (3 * g + 2) // 16})
    # block u's window: groups g0 .. g0 + 5, g0 = 16u // 3
    lo = (3 * g) // 16
    return [u for u in range(max(lo - 2, 0), lo + 2) if 16 * u // 3 <= g <= 16 * u // 3 + 5]


def where(pos: int) -> str:
    """`pos` as line:column, one-pass tile / workgroup / lane, scan trip / lane."""
    line, col = divmod(pos, LINE_CHARS)
    tile = line // DEC_LINES
    lanes = [u % (DEC_BYTES // 16) for u in one_pass_blocks(pos)]
    return (f"{line}:{col} tile {tile} wg {tile // DEC_TILES_PER_GROUP} lane {lanes} "
            f"trip {pos // SCAN_CHARS} lane {pos % SCAN_CHARS // 16}.{pos % 16}")


# -------------------------------------------------------------------- corpora
class Corpus:
    """Texts for one lbf_b64_verify_batch call.  Entry i: `texts[i]` arrives
    for the chunk `chunks[i]` (its digest is the expected one unless
    digest_ok[i] is false) into a slot of caps[i] bytes; tphase / sphase are
    the text's and the slot's start mod 16 (None: wherever the gaps put it);
    desc[i] says what the entry is, for a failing assertion."""

    def __init__(self, name):
        self.name = name
        self.texts, self.chunks, self.caps, self.desc = [], [], [], []
        self.tphase, self.sphase, self.digest_ok = [], [], []

    def add(self, text, chunk, desc, cap=None, tphase=None, sphase=None, digest_ok=True):
        self.texts.append(bytes(text))
        self.chunks.append(bytes(chunk))
        self.caps.append(len(chunk) if cap is None else cap)
        self.tphase.append(tphase)
        self.sphase.append(sphase)
        self.desc.append(f"{self.name}[{len(self.desc)}] {desc}")
        self.digest_ok.append(digest_ok)

    def __len__(self):
        return len(self.texts)

    def expected(self):
        """Per entry, from `decode` alone: (decoded bytes w, reported length,
        verdict).  The verdict is 1 when w is the chunk, whose size is the
        slot's (ChunkMethods.cpp:156), and the expected digest is the chunk's."""
        out = []
        for t, d, cap, ok in zip(self.texts, self.chunks, self.caps, self.digest_ok):
            w = decode(t)
            out.append((w, len(w) if len(w) <= cap else cap + 1, w == d and cap == len(d) and ok))
        return out

    def layout_counts(self):
        """(texts the one-pass decode keeps, texts it hands to the general one)."""
        one = sum(is_encoder_layout(t) for t in self.texts)
        return one, len(self.texts) - one


@functools.lru_cache(maxsize=None)
def chunk_bytes(n: int, seed: int = 0) -> bytes:
    return np.random.default_rng(1000 + 7 * n + seed).integers(0, 256, n, dtype=np.uint8).tobytes()


PERIOD_SIZES = (864, 865, 866)      # 16 lines: no tail, "xx==", "xxx="
EDGE_SIZES = (20674, 20675)         # five decode tiles and a part, two workgroups, seven scan trips


def period_corpus(kind: str, step: int = 1) -> Corpus:
    """Test 1: `kind` at every character position of 16-line texts (one period
    of lines against six-group blocks, 8 lines, and against 16-character lanes,
    16 lines), and the undamaged texts."""
    c = Corpus(f"period/{kind}")
    for n in PERIOD_SIZES:
        d = chunk_bytes(n)
        t = xmlrpc_text(d)
        c.add(t, d, f"{n} B undamaged")
        for p in positions(len(t), kind)[::step]:
            c.add(damage(t, kind, p), d, f"{n} B {kind} at {p} = {where(p)}")
    return c


def edge_positions(text_len: int):
    """Test 2's places in a text of an EDGE_SIZES chunk: the lines on both
    sides of the first tile edge, of the workgroup edge and of a later tile
    edge, 17 characters to both sides of scan trips 1, 2 and 6, the last 80."""
    ps = set()
    for first in (DEC_LINES - 1, DEC_LINES * DEC_TILES_PER_GROUP - 1, 5 * DEC_LINES - 1):
        ps.update(range(first * LINE_CHARS, (first + 2) * LINE_CHARS))
    for k in (1, 2, 6):
        ps.update(range(SCAN_CHARS * k - 17, SCAN_CHARS * k + 18))
    ps.update(range(text_len - 80, text_len))
    return sorted(ps)


def edge_corpus(kind: str) -> Corpus:
    c = Corpus(f"edges/{kind}")
    for n in EDGE_SIZES:
        d = chunk_bytes(n)
        t = xmlrpc_text(d)
        c.add(t, d, f"{n} B undamaged")
        ps = edge_positions(len(t))
        if kind == "cut" or kind.startswith("ins_"):
            ps = ps + [len(t)]
        for p in ps:
            c.add(damage(t, kind, p), d, f"{n} B {kind} at {p} = {where(p)}")
    return c


_D, _G = DEC_BYTES, DEC_BYTES * DEC_TILES_PER_GROUP
DISAGREE_PAIRS = ([(0, 1), (0, _G + 5), (2 * _D, 0), (40, _D), (_D - 1, _D), (_D, _D - 1), (_D + 1, _D),
                   (_D, 2 * _D + 7), (100, _G + _D + 3), (_G + 10, 50), (_G + _D, _G + _D - 1), (_G + _D, _G + _D + 1)]
                  + [(2 * _G + 100, 2 * _G + 100 - k) for k in (1, 15, 16)])


def disagree_corpus() -> Corpus:
    """Test 3: (decoded length L, slot C) pairs a truncated or over-long frame
    gives, on both decode paths, slots at 0 and 5 and texts at 0 and 3 mod 16.
    The chunk the receiver expects is C bytes of the same stream, so the
    verdict is 1 only where L == C."""
    c = Corpus("disagree")
    stream = chunk_bytes(2 * _G + 200, seed=3)
    for L, C in DISAGREE_PAIRS:
        for path in ("one-pass", "general"):
            for sphase in (0, 5):
                for tphase in (0, 3):
                    t = xmlrpc_text(stream[:L])
                    if path == "general":
                        t = b"\x01" + t
                    c.add(t, stream[:C], f"L={L} C={C} {path} slot%16={sphase} text%16={tphase}",
                          cap=C, tphase=tphase, sphase=sphase)
    return c


def _alpha_stream(n: int, seed: int) -> bytes:
    """n alphabet characters, no separators."""
    idx = np.random.default_rng(seed).integers(0, 64, n)
    return np.frombuffer(ALPHABET, dtype=np.uint8)[idx].tobytes()


def scan_families():
    """Test 4: {family: [(text, what)]}, every text outside the encoder's layout."""
    fam = {}
    # successive 16-character lanes hold 0, 1, ..., 16 valid characters
    woven = []
    for v, lanes in enumerate((600, 1000)):
        rng = np.random.default_rng(50 + v)
        t = bytearray()
        for lane in range(lanes):
            nv = lane % 17
            cs = [JUNK[int(rng.integers(0, len(JUNK)))]] * 16
            for k in rng.permutation(16)[:nv]:
                cs[int(k)] = ALPHABET[int(rng.integers(0, 64))]
            t += bytes(cs)
        for cutoff in (len(t), len(t) - 7):
            woven.append((bytes(t[:cutoff]), f"woven {lanes} lanes, {cutoff} characters"))
    fam["woven"] = woven
    # a run of junk longer than a scan trip: whole trips that add nothing
    base = xmlrpc_text(chunk_bytes(9000, seed=5))
    run = bytes(JUNK[k % len(JUNK)] for k in range(2 * SCAN_CHARS + 9))
    fam["junk-run"] = [(run + base, "junk run first"), (base[:5000] + run + base[5000:], "junk run in the middle"),
                       (base + run, "junk run last"),
                       (run[:SCAN_CHARS + 1] + base[:4097] + run + base[4097:], "two junk runs")]
    # the first '=' at index 4096k + j of a text without junk (stream index = text index)
    eqs = []
    for k in (1, 2):
        for j in range(-5, 6):
            q = SCAN_CHARS * k + j
            t = bytearray(_alpha_stream(q + 1 + 5300, 60 + 16 * k + j))
            t[q] = ord("=")
            for later in (q + 1, q + 700, q + 4500, len(t) - 1):
                if later != q + 1 or j % 2:
                    t[later] = ord("=")
            eqs.append((bytes(t), f"first '=' at {q} (q % 4 = {q % 4}), more behind it"))
    fam["first-eq"] = eqs
    # two '=' in one trip, in different waves (1,024 characters each): the lower index wins
    two = []
    for n, (trip, a, b) in enumerate(((0, 70, 3000), (1, 1030, 2050), (1, 5, 4090), (2, 1023, 1024),
                                      (2, 2047, 3073), (0, 1025, 2048), (1, 3071, 3072), (2, 100, 4000))):
        t = bytearray(_alpha_stream(3 * SCAN_CHARS + 50, 90 + n))
        t[trip * SCAN_CHARS + a] = t[trip * SCAN_CHARS + b] = ord("=")
        two.append((bytes(t), f"'=' at {a} and {b} of trip {trip} (waves {a // 1024} and {b // 1024})"))
    fam["two-eq"] = two
    # lengths around whole trips (a junk character in front breaks the layout)
    fam["length"] = [(b"\x7f" + _alpha_stream(SCAN_CHARS * k + d - 1, 120 + 8 * k + d), f"length {SCAN_CHARS * k + d}")
                     for k in (1, 2) for d in (-16, -15, -1, 0, 1, 15, 16, 17)]
    # complete group counts around whole pass-2 trips, with 0..3 characters of a group cut short behind them
    groups = []
    for k in (1, 2, 3):
        for d in range(-1, 6):
            g = SCAN_GROUPS * k + d
            r = (k + d) % 4
            groups.append((b"\n" + _alpha_stream(4 * g + r, 150 + 8 * k + d),
                           f"{g} complete groups and {r} characters"))
    fam["groups"] = groups
    return fam


CAP_DELTAS = (0, -1, -5, 9)


def scan_corpus() -> Corpus:
    """Test 4: the families on rotating text and slot phases (0..3) and slot
    sizes L, L - 1, L - 5, L + 9 around the decoded length L.  The chunk the
    receiver expects is the reference decode itself, so the verdict is 1
    exactly where the slot is L bytes."""
    c = Corpus("scan")
    for name, texts in scan_families().items():
        for i, (t, what) in enumerate(texts):
            w = decode(t)
            cap = max(0, len(w) + CAP_DELTAS[(i + i // 4) % 4])
            c.add(t, w, f"{name}: {what}; L={len(w)} cap={cap}", cap=cap, tphase=i % 4,
                  sphase=(3 * i + i // 4) % 4)
    return c


def slices_corpus(extra: int = 300) -> Corpus:
    """Test 5: one launch slice and `extra` more chunks of 0..60 bytes; every
    7th text has a junk character inserted, every 11th expected digest is wrong."""
    c = Corpus("slices")
    n = CHUNKS_PER_LAUNCH + extra
    rng = np.random.default_rng(77)
    sizes = rng.integers(0, 61, n)
    stream = rng.integers(0, 256, int(sizes.sum()), dtype=np.uint8).tobytes()
    at = 0
    for i in range(n):
        d = stream[at:at + int(sizes[i])]
        at += int(sizes[i])
        t = xmlrpc_text(d)
        what = f"{len(d)} B"
        if i % 7 == 0:
            p = (i // 7) % (len(t) + 1)
            t = damage(t, "ins_junk", p)
            what += f" junk inserted at {p}"
        c.add(t, d, what, digest_ok=i % 11 != 0)
    return c


def encode_cases():
    """Test 6: [(size, source phase mod 16, text slot phase mod 16)]: sizes on
    both sides of the encode's tile edges (6,048 bytes; two tiles to a
    workgroup) and of its line edges, the first two tile edges at every source
    phase, the rest on rotating phases."""
    cases, n = [], 0
    for k in (1, 2, 3, 4):
        for d in range(-3, 4):
            for phase in (range(16) if k <= 2 else [n % 16]):
                cases.append((ENC_BYTES * k + d, phase, (0, 1, 8, 15)[n % 4]))
                n += 1
    for j in (0, 1, 17, 18, 112):
        for d in (0, 1, 2):
            cases.append((54 * j + d, (5 * n + 3) % 16, (0, 1, 8, 15)[n % 4]))
            n += 1
    return cases

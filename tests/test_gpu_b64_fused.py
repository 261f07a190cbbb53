"""The fused route of the piecewise base64 decode on the GPU: the line, flat
and scan stages of a piece in one launch (bitflood_amd/csrc/
b64_update_fused.hip: b64_update_fused_kernel, lbf_set_b64_fused), with
lbf_set_b64_lines / lbf_set_b64_flat as its stage mask.

Expected values come from tests/wire_layouts.py and tests/wire_piece_model.py
(pinned to xmlrpc++'s recorded answers), tests/wire_flat_model.py and
tests/wire_line_model.py and hashlib, never from a GPU path.  Every piecewise
call is checked whole, as in tests/test_gpu_b64_update.py (whose Chain, Feed
and DeviceFeed run the rounds): both state arrays, every byte of the arena --
0xEE wherever nothing was decoded -- lengths, verdicts and the counters
(tests/test_gpu_b64_flat.py's FlatFeed).  run_both feeds the same rounds to the
unfused route with the same stage mask and holds the two together: bytes, both
state arrays, lengths, verdicts, and what each path took, to the character.
"""
import base64
import functools

import numpy as np
import pytest

from bitflood_amd import B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, _capi, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import wire_flat_model as F
from tests import wire_layouts as W
from tests import wire_piece_model as M
from tests.test_gpu_b64_flat import HURT, FlatFeed, hurt
from tests.test_gpu_b64_update import FILL, Chain, DeviceFeed, Feed, sha1

pytestmark = pytest.mark.gpu

T = F.TILE_BYTES
TILE_TEXT = {"xmlrpc": W.DEC_TEXT, "unbroken": F.TILE_TEXT}  # 5,256 characters of lines, 5,184 unbroken
ENCODE = {"xmlrpc": W.xmlrpc_text, "unbroken": F.text}
LAYOUTS = ("xmlrpc", "unbroken")
SIZES = (0, 1, 2, 3, 55, 57, 58, 864)
BIG = 5 * T + 1000
GIB = 1 << 30


@pytest.fixture(autouse=True)
def fused_on():
    before = H.set_b64_fused(True)
    yield
    H.set_b64_fused(before)


@pytest.fixture(params=[(True, True), (True, False), (False, True), (False, False)],
                ids=["lines+flat", "lines", "flat", "scan"])
def mask(request):
    """The stage mask: (line stage, flat stage)."""
    lines, flat = request.param
    before = H.set_b64_lines(lines), H.set_b64_flat(flat)
    yield request.param
    H.set_b64_lines(before[0])
    H.set_b64_flat(before[1])


def counters(hasher):
    u, f = hasher.b64_update_stats(), hasher.b64_flat_stats()
    return np.array([u["line_chars"], u["scan_chars"], f["flat_chars"]], dtype=np.int64)


def run_both(hasher, chains, mask, sphase=None, tphase=None, undamaged=True):
    """Every round on the fused route (a FlatFeed: everything against the
    models, the counters against the stage mask) and on the unfused one (a Feed:
    everything against the models), then one against the other."""
    lines, flat = mask
    fused = FlatFeed(chains, sphase, tphase, undamaged=undamaged, lines=lines, flat=flat)
    plain = Feed(chains, sphase, tphase)
    for r in range(fused.rounds):
        total = sum(len(c.pieces[r]) for c in chains if r < len(c.pieces))
        got = []
        for feed, on in ((fused, True), (plain, False)):
            assert H.set_b64_fused(on) is True
            try:
                c0 = counters(hasher)
                sizes, ver = feed.run_round(hasher, r)
                took = counters(hasher) - c0
            finally:
                H.set_b64_fused(True)
            feed.check_sha([r >= len(c.pieces) - 1 for c in chains])
            assert took[0] + took[1] == total and 0 <= took[2] <= took[1], (r, on, took.tolist(), total)
            got.append((sizes, ver, took))
        assert got[0][2].tolist() == got[1][2].tolist(), (r, got[0][2].tolist(), got[1][2].tolist())
        assert got[0][0].tolist() == got[1][0].tolist() and got[0][1].tolist() == got[1][1].tolist(), r
        assert fused.out.tobytes() == plain.out.tobytes(), r
        assert fused.b64.tobytes() == plain.b64.tobytes(), r
        assert not M.sha_records_differ(fused.sha, plain.sha), r
    for feed in (fused, plain):  # every chain has had its final piece: both records as new
        assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()
        assert feed.sha.tobytes() == new_states(len(chains)).tobytes()
    return fused


# ------------------------------------------------------------ 1. every cut of small texts
@functools.lru_cache(maxsize=None)
def _small_chains(layout):
    chains = []
    for n in SIZES:
        d = W.chunk_bytes(n)
        t = ENCODE[layout](d)
        chains += [Chain([t[:a], t[a:]], chunk=d, desc=f"{layout} {n} B cut at {a}") for a in range(len(t) + 1)]
    assert all(c.verdict for c in chains)
    return chains


@pytest.mark.parametrize("sphase,tphase", [(0, 0), (5, 3)])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_every_cut_of_small_texts(hasher, mask, layout, sphase, tphase):
    """Less than one tile a piece: every carry, every output phase, both sides
    of the '=' group, pieces too short to complete a group; on both routes."""
    feed = run_both(hasher, _small_chains(layout), mask, sphase, tphase)
    if mask[1] and (layout == "unbroken" or not mask[0]):  # the flat stage is not behind a line stage that took it all
        assert feed.flat_chars > 0


# ------------------------------------------------------------ 2. tile edges
@functools.lru_cache(maxsize=None)
def big_text(layout, seed=0):
    d = W.chunk_bytes(BIG, seed=seed)
    return d, ENCODE[layout](d)


def _edge_cuts(n, tile):
    return sorted(set(range(0, 147)) | set(range(tile - 80, tile + 81)) | set(range(n - 160, n + 1)))


@functools.lru_cache(maxsize=None)
def _edge_chains(layout):
    d, t = big_text(layout)
    return [Chain([t[:a], t[a:]], chunk=d, desc=f"{layout} cut at {a}") for a in _edge_cuts(len(t), TILE_TEXT[layout])]


@pytest.mark.parametrize("layout", LAYOUTS)
def test_two_piece_cuts_around_tile_edges(hasher, mask, layout):
    """Five tiles and a part, cut at every character of the first 147, around
    the layout's first tile edge and in the last 160 characters; on both routes."""
    chains = _edge_chains(layout)
    feed = run_both(hasher, chains, mask, sphase=5, tphase=3)
    if mask[1] and (layout == "unbroken" or not mask[0]):  # the flat stage has tiles of its own
        floor = len(big_text(layout)[1]) - TILE_TEXT[layout] - 200 if layout == "unbroken" else 0
        assert feed.flat_chars > len(chains) * floor


@pytest.mark.parametrize("layout", LAYOUTS)
def test_three_piece_cuts_through_the_device_resident_launch(mask, layout):
    """lbf_b64_update_launch: the cuts around the first tile edge, three pieces
    a chain, everything in device buffers on a side stream."""
    d, t = big_text(layout, seed=1)
    tile = TILE_TEXT[layout]
    chains = [Chain([t[:a], t[a:a + tile + e], t[a + tile + e:]], chunk=d, desc=f"{layout} cuts at {a}, {e}")
              for a in (0, 1, 2, 3, 37) for e in range(-12, 13)]
    feed = Feed(chains, sphase=3 if mask[0] else 12, tphase=9)
    dev = DeviceFeed(feed, len(chains), max(feed.texts(range(len(chains)), r)[0].size for r in range(3)))
    try:
        for r in range(3):
            dev.run_round(r)
    finally:
        dev.close()
    assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()
    assert feed.sha.tobytes() == new_states(len(chains)).tobytes()


# ------------------------------------------------------------ 3. stage hand-over
def mixed_text(d: bytes, c1: int, c2: int):
    """One chunk's text in three layouts: the encoder's lines for the first tile
    and a part, then unbroken text, then a CR LF pair after every 76 characters
    (the scan's share).  The first boundary falls c1 characters into a group,
    the second c2: a chain cut there carries that many sextets."""
    s = base64.b64encode(d)
    body = s.rstrip(b"=")
    a = 72 * 80 + 20 + c1
    b = a - c1 + 4 * 1500 + c2
    lines = b"".join(body[k:min(k + 72, a)] + (b" " if k + 72 <= a else b"") for k in range(0, a, 72))
    rest = body[b:] + s[len(body):]
    crlf = b"".join(rest[k:k + 76] + b"\r\n" for k in range(0, len(rest), 76))
    return lines, body[a:b], crlf


@functools.lru_cache(maxsize=None)
def _mixed_chains():
    chains = []
    for c1, c2 in ((0, 1), (1, 2), (2, 3), (3, 0)):
        d = W.chunk_bytes(BIG, seed=30 + c1)
        p1, p2, p3 = mixed_text(d, c1, c2)
        t = p1 + p2 + p3
        assert W.decode(t) == d
        after1, _ = M.update(M.init(), p1)
        after2, _ = M.update(after1, p2)
        assert (len(after1[1]), len(after2[1])) == (c1, c2)
        desc = f"mixed, carries {c1} and {c2}"
        chains.append(Chain([t[:100], t[100:-50], t[-50:]], chunk=d, desc=desc + ", one piece spans all three"))
        chains.append(Chain([p1, p2, p3], chunk=d, desc=desc + ", a piece a layout"))
        chains.append(Chain([p1[:3001], p1[3001:], p2, p3[:7000], p3[7000:]], chunk=d, desc=desc + ", five pieces"))
        chains.append(Chain([t], chunk=d, desc=desc + ", whole"))
    assert all(c.verdict for c in chains)
    return chains


def test_stage_hand_over_inside_a_piece_and_across_a_chain(hasher, mask):
    """A text that changes layout twice: cut so that one piece spans all three
    layouts (the three stages each take their share of one piece, the record in
    registers between them), and so that each boundary is a piece boundary with
    0..3 sextets carried across it.  The whole-text decode is the arbiter."""
    feed = run_both(hasher, _mixed_chains(), mask, sphase=7, tphase=2, undamaged=False)
    if mask[1]:  # the unbroken part, about 6,000 characters, is a piece of its own in two chains of each four
        assert feed.flat_chars >= 4 * 2 * 5900


# ------------------------------------------------------------ 4./6. one hand-built launch
class Piece:
    """One piece of a hand-built launch.  `state` is the chain's state as the
    kernels read it and `prefix` what it has decoded into the slot so far (the
    SHA record has absorbed it); `raw` forges the record's fields instead, and
    then only the record, the slot and the tables are checked.  cap None: what
    the chain decodes to after this piece."""

    def __init__(self, text, state=M.init(), prefix=b"", cap=None, fin=False, raw=None, digest_ok=True, desc=""):
        self.text, self.state, self.prefix, self.fin, self.raw, self.desc = text, state, prefix, fin, raw, desc
        self.refused = cap is not None and cap > GIB
        self.after, new = M.update(state, text)
        self.new = b"" if self.refused else new
        self.total = state[0] + len(self.new)  # the chain's byte count behind the piece
        self.cap = self.total if cap is None else cap
        self.lo, self.hi = min(state[0], self.cap), max(min(self.total, self.cap), min(state[0], self.cap))
        self.sofar = prefix + new if raw is None else None
        self.digest = sha1((prefix + new)[:self.cap]) if raw is None else bytes(20)
        self.expected = self.digest if digest_ok else bytes([self.digest[0] ^ 1]) + self.digest[1:]


def mid(first: bytes, **kw):
    """A chain that has had `first`: (state, prefix) for Piece."""
    state, prefix = M.update(M.init(), first)
    return dict(state=state, prefix=prefix, **kw)


def run_launch(pieces, skipped_text=b"QUJD"):
    """pieces[k] continues chain k in one lbf_b64_update_launch; one more piece
    names chain len(pieces), which does not exist.  Everything the launch may
    write is checked: the arena (FILL around and between slots, below the
    chain's position and past what it decoded), both record arrays and the guard
    record behind each, the piece table, lengths, digests and verdicts."""
    lib = _capi.load()
    n_states = len(pieces)
    n = n_states + 1
    room = max(p.cap for p in pieces if not p.refused) + 240
    slot = (64 + room * np.arange(n, dtype=np.uint64) + np.arange(n, dtype=np.uint64) % 16).astype(np.uint64)
    out = np.full(64 + room * n + 16, FILL, dtype=np.uint8)
    b64, sha = new_b64_states(n_states + 1), new_states(n_states + 1)
    b64.view(np.uint8).reshape(-1, 16)[n_states] = FILL
    sha.view(np.uint8).reshape(-1, 96)[n_states] = FILL
    want_b64, want_sha = new_b64_states(n_states), new_states(n_states)
    for k, p in enumerate(pieces):
        if p.raw is None:
            b64[k] = M.b64_record(p.state)
            sha[k:k + 1] = M.sha_records([M.sha_state(p.prefix, p.cap)], STATE_DTYPE)
            out[int(slot[k]):int(slot[k]) + p.lo] = np.frombuffer(p.prefix[:p.lo], np.uint8)
        else:
            for field, v in p.raw.items():
                b64[field][k] = v
    want_out = out.copy()
    for k, p in enumerate(pieces):
        at = int(slot[k])
        want_out[at + p.lo:at + p.hi] = np.frombuffer(p.new[:p.hi - p.lo], np.uint8)
        if p.fin:
            continue  # both records as new
        if not p.refused:
            want_b64[k] = M.b64_record((min(p.after[0], 1 << 61), p.after[1], p.after[2]))
        else:
            want_b64[k] = b64[k]  # a refused piece that is not final leaves the record
        if p.raw is None:
            want_sha[k:k + 1] = M.sha_records([M.sha_state(p.sofar if not p.refused else p.prefix, p.cap)], STATE_DTYPE)
    texts = [p.text for p in pieces] + [skipped_text]
    toff = np.cumsum([0] + [len(t) + 16 + k % 5 for k, t in enumerate(texts[:-1])]).astype(np.uint64)
    text = np.zeros(int(toff[-1]) + len(texts[-1]) + 16, np.uint8)
    for k, t in enumerate(texts):
        text[int(toff[k]):int(toff[k]) + len(t)] = np.frombuffer(t, np.uint8)
    E4, E8 = 0xEEEEEEEE, 0xEEEEEEEEEEEEEEEE
    host = dict(b64=b64, sha=sha, so=np.arange(n, dtype=np.uint32), text=text, toff=toff,
                tlen=np.array([len(t) for t in texts], np.uint32),
                fin=np.array([p.fin for p in pieces] + [1], np.uint8), out=out, ooff=slot,
                caps=np.array([p.cap for p in pieces] + [64], np.uint32), osz=np.full(n, E4, np.uint32),
                dig=np.full(20 * n, FILL, np.uint8),
                exp=np.frombuffer(b"".join(p.expected for p in pieces) + bytes(20), np.uint8).copy(),
                ver=np.full(n, FILL, np.uint8), poff=np.full(n, E8, np.uint64), psz=np.full(n, E4, np.uint32))
    bufs = {k: DeviceBuffer(v.nbytes) for k, v in host.items()}
    try:
        for k, v in host.items():
            bufs[k].upload(v)
        H.b64_update_launch(bufs["b64"], bufs["sha"], n_states, bufs["so"], bufs["text"], bufs["toff"], bufs["tlen"],
                            bufs["fin"], n, bufs["out"], bufs["ooff"], bufs["caps"], bufs["osz"], bufs["dig"],
                            bufs["exp"], bufs["ver"], bufs["poff"], bufs["psz"])
        _capi.check(lib.lbf_device_synchronize())
        got = {k: bufs[k].download(host[k].nbytes) for k in ("out", "b64", "sha", "dig", "ver")}
        osz = bufs["osz"].download(4 * n, dtype=np.uint32)
        psz = bufs["psz"].download(4 * n, dtype=np.uint32)
        poff = bufs["poff"].download(8 * n, dtype=np.uint64)
    finally:
        for b in bufs.values():
            b.free()
    wrong = np.flatnonzero(got["out"] != want_out)
    assert wrong.size == 0, (wrong[:8].tolist(), [int(x) for x in slot])
    b2, s2 = got["b64"].view(B64_STATE_DTYPE), got["sha"].view(STATE_DTYPE)
    assert b2[n_states].tobytes() == bytes([FILL]) * 16 and s2[n_states].tobytes() == bytes([FILL]) * 96
    dig = got["dig"].reshape(n, 20)
    # the piece that names no chain: nothing written for it
    assert (psz[n_states], poff[n_states], osz[n_states], got["ver"][n_states]) == (E4, E8, E4, FILL)
    assert (dig[n_states] == FILL).all()
    for k, p in enumerate(pieces):
        assert b2[k].tobytes() == want_b64[k].tobytes(), (k, p.desc, b2[k], want_b64[k])
        assert psz[k] == p.hi - p.lo <= p.cap - p.lo or p.refused, (k, p.desc, int(psz[k]), p.hi - p.lo)
        assert poff[k] == (0 if p.refused else int(slot[k]) + p.lo) and (not p.refused or psz[k] == 0), (k, p.desc)
        if p.raw is None or p.fin:
            assert not M.sha_records_differ(s2[k:k + 1], want_sha[k:k + 1]), (k, p.desc, s2[k], want_sha[k])
        if not p.fin:
            assert osz[k] == E4 and got["ver"][k] == FILL and (dig[k] == FILL).all(), (k, p.desc)
            continue
        size = 0 if p.refused else p.total if p.total <= p.cap else p.cap + 1
        assert osz[k] == size, (k, p.desc, int(osz[k]), size)
        if p.raw is None and not p.refused:
            assert dig[k].tobytes() == p.digest, (k, p.desc)
            assert got["ver"][k] == int(p.total == p.cap and p.expected == p.digest), (k, p.desc)
        else:
            assert got["ver"][k] == 0, (k, p.desc)  # all-zero `expected`, or refused
    return psz


def test_per_piece_routing_in_one_launch(mask):
    """Encoder-layout chains, unbroken chains, chains whose text changes layout
    and chains that have ended, side by side in one device-resident launch, each
    piece routed by its own text; a piece that names no chain is skipped with
    nothing written, a chunk over 1 GiB is refused, and the guard bytes around
    and between the slots stay."""
    d = [W.chunk_bytes(2 * T + 700 + 3 * k, seed=40 + k) for k in range(4)]
    x, u = [W.xmlrpc_text(b) for b in d], [F.text(b) for b in d]
    p1, p2, p3 = mixed_text(W.chunk_bytes(BIG, seed=44), 2, 1)
    ended = M.update(M.init(), u[3])
    assert ended[0][2]
    pieces = [
        Piece(x[0], fin=True, desc="encoder layout, whole"),
        Piece(u[0], fin=True, desc="unbroken, whole"),
        Piece(x[1][101:6000], **mid(x[1][:101]), cap=len(d[1]), desc="encoder layout, a middle piece"),
        Piece(u[1][101:6000], **mid(u[1][:101]), cap=len(d[1]), desc="unbroken, a middle piece"),
        Piece(x[2][50:], **mid(x[2][:50]), fin=True, desc="encoder layout, the final piece"),
        Piece(u[2][50:], **mid(u[2][:50]), fin=True, digest_ok=False, desc="unbroken, final, wrong digest"),
        Piece((p1 + p2 + p3)[70:], **mid(p1[:70]), fin=True, desc="three layouts in one piece"),
        Piece(p2 + p3[:3000], **mid(p1), cap=BIG, desc="unbroken, then CR LF text"),
        Piece(x[3][:500], state=ended[0], prefix=ended[1], cap=len(d[3]), desc="text for a chain that has ended"),
        Piece(b"", state=ended[0], prefix=ended[1], cap=len(d[3]), fin=True, desc="ended, the empty final piece"),
        Piece(u[0], cap=GIB + 1, desc="over 1 GiB"),
        Piece(x[0], **mid(x[0][:40]), cap=GIB + 1, fin=True, desc="over 1 GiB, final"),
        Piece(b"", desc="an empty piece"),
    ]
    psz = run_launch(pieces)
    assert psz[0] == psz[1] == len(d[0]) and psz[8] == 0 and psz[6] == BIG - len(M.update(M.init(), p1[:70])[1])


def test_forged_device_records(mask):
    """Records the launch cannot read, forged, two tiles and a part of text a
    piece in either layout: ncarry = 7 counts & 3 and the carry's high bits are
    masked; `decoded` = 2^63 is clamped to 2^61, no multiple of 3, left to the
    scan and writes nothing; `decoded` = 7 (not a multiple of 3) is the scan's
    too; ended = 255 ignores the text.  Nothing outside the slot and the records
    is written."""
    cap = 9000
    body = {"xmlrpc": W.xmlrpc_text(W.chunk_bytes(3 * T, seed=12)), "unbroken": F.text(W.chunk_bytes(3 * T, seed=12))}
    pieces = []
    for layout in LAYOUTS:
        t = body[layout][:2 * TILE_TEXT[layout] + 301]
        three = (63, 63, 63)
        pieces += [
            Piece(t, state=(0, three, False), cap=cap, raw=dict(ncarry=7, carry=0xFFFFFFFF), desc=f"{layout} ncarry 7"),
            Piece(t, state=(96, three, False), cap=cap, fin=True, raw=dict(decoded=96, ncarry=7, carry=0xFFFFFFFF),
                  desc=f"{layout} ncarry 7 at 96, final"),
            Piece(t, state=(54, (5, 9), False), cap=cap,
                  raw=dict(decoded=54, ncarry=2, carry=5 | (9 << 6) | (0xABC << 12)),
                  desc=f"{layout} carry with high bits"),
            Piece(t, state=(1 << 61, (), False), cap=cap, raw=dict(decoded=1 << 63), desc=f"{layout} decoded 2^63"),
            Piece(t, state=(1 << 61, (), False), cap=cap, fin=True, raw=dict(decoded=1 << 63),
                  desc=f"{layout} decoded 2^63, final"),
            Piece(t, state=(7, (), False), cap=cap, raw=dict(decoded=7), desc=f"{layout} decoded 7"),
            Piece(t, state=(3 << 40, (), False), cap=cap, raw=dict(decoded=3 << 40), desc=f"{layout} decoded 3 * 2^40"),
            Piece(t, state=(54, (), True), cap=cap, raw=dict(decoded=54, ended=255), desc=f"{layout} ended 255"),
        ]
    psz = run_launch(pieces)
    assert psz[0] > 2 * T and psz[3] == psz[6] == psz[7] == 0 and psz[8 + 3] == psz[8 + 6] == psz[8 + 7] == 0


# ------------------------------------------------------------ 5. damage
def _tile_places(tile, lead):
    """The first, middle and last character of the chunk's second tile and of the
    one after it, as places in a piece that starts `lead` characters in."""
    return [k * tile - lead + at for k in (1, 2) for at in (0, tile // 2, tile - 1)]


@functools.lru_cache(maxsize=None)
def _damage_chains(kind, layout):
    d, t = big_text(layout, seed=2 + HURT.index(kind))
    first, rest = t[:101], t[101:]
    chains = [Chain([first, rest], chunk=d, desc=f"{layout} undamaged")]
    chains += [Chain([first, hurt(rest, kind, p)], cap=len(d), chunk=d, desc=f"{layout} {kind} at {p} of piece 2")
               for p in _tile_places(TILE_TEXT[layout], 101)]
    return chains


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("kind", HURT)
def test_damage_stays_unwritten(hasher, mask, kind, layout):
    """Damage at the first, middle and last character of a tile and of the tile
    after it.  Device-resident, the arena read back whole after each launch: the
    model's bytes below the new `decoded`, 0xEE everywhere else, whatever a tile
    that held the damage had decoded before it showed.  Then the batch call, on
    both routes, with the counters."""
    chains = _damage_chains(kind, layout)
    feed = Feed(chains, sphase=9, tphase=6)
    dev = DeviceFeed(feed, len(chains), max(feed.texts(range(len(chains)), r)[0].size for r in range(2)))
    try:
        dev.run_round(0)
        dev.run_round(1)
    finally:
        dev.close()
    assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()
    run_both(hasher, chains, mask, sphase=9, tphase=6, undamaged=False)


# ------------------------------------------------------------ 6. slot and length disagree
@pytest.mark.parametrize("layout", LAYOUTS)
def test_slot_and_length_disagree(hasher, mask, layout):
    """A text of L bytes into slots of L - 1, L - 5, L - 17, L + 9 and one that
    ends inside the first block of a tile, as three pieces: nothing at or past
    cap (the guards behind every slot stay), out_sizes = cap + 1 and verdict 0
    where the text decodes to more, fewer bytes than cap where it decodes to
    less, and the record counts on past the slot."""
    d, t = big_text(layout, seed=7)
    n = len(d)
    chains = []
    for cap in (n - 1, n - 5, n - 17, n + 9, 2 * T + 7, n):
        for a, b in ((5000, 15000), (len(ENCODE[layout](bytes(cap // 3 * 3 - 300))) if cap < n else 9000, len(t) - 50),
                     (1, 74)):
            chains.append(Chain([t[:a], t[a:b], t[b:]], cap=cap, desc=f"{layout} cap {cap} of {n}, cuts at {a}, {b}"))
            assert chains[-1].size == (n if n <= cap else cap + 1) and chains[-1].verdict == (cap == n)
    assert any(len(c.want) > c.cap for c in chains) and any(len(c.want) < c.cap for c in chains)
    run_both(hasher, chains, mask, sphase=7, tphase=1)


# ------------------------------------------------------------ 7. the device-resident launch, route against route
def test_device_resident_launch_equals_the_unfused_route(mask):
    """The mixed-layout chains and tile-edge cuts of both layouts through
    lbf_b64_update_launch on both routes: the arena, both record arrays,
    out_sizes, digests, verdicts and the piece table the hash read are the same,
    call by call."""
    chains = list(_mixed_chains())
    for layout in LAYOUTS:
        d, t = big_text(layout, seed=1)
        chains += [Chain([t[:a], t[a:a + TILE_TEXT[layout] + e], t[a + TILE_TEXT[layout] + e:]], chunk=d,
                         desc=f"{layout} cuts at {a}, {e}") for a in (1, 37) for e in (-5, 0, 6)]
    seen = []
    for on in (True, False):
        assert H.set_b64_fused(on) is True
        try:
            feed = Feed(chains, sphase=11, tphase=5)
            rounds = range(feed.rounds)
            live = lambda r: [k for k, c in enumerate(chains) if r < len(c.pieces)]  # noqa: E731
            dev = DeviceFeed(feed, len(chains), max(feed.texts(live(r), r)[0].size for r in rounds))
            try:
                for r in rounds:
                    dev.run_round(r)
                    m = len(live(r))
                    seen.append((on, r, feed.out.tobytes(), feed.b64.tobytes(), feed.sha.tobytes(),
                                 dev.bufs["osz"].download(4 * m).tobytes(), dev.bufs["dig"].download(20 * m).tobytes(),
                                 dev.bufs["ver"].download(m).tobytes(), dev.bufs["poff"].download(8 * m).tobytes(),
                                 dev.bufs["psz"].download(4 * m).tobytes()))
            finally:
                dev.close()
        finally:
            H.set_b64_fused(True)
    half = len(seen) // 2
    for a, b in zip(seen[:half], seen[half:]):
        assert a[0] and not b[0] and a[1] == b[1]
        for what, x, y in zip(("out", "b64", "sha", "out_sizes", "digests", "verdicts", "piece_offsets", "piece_sizes"),
                              a[2:], b[2:]):
            assert x == y, (a[1], what)


# ------------------------------------------------------------ 8. final pieces
@pytest.mark.parametrize("layout", LAYOUTS)
def test_a_chain_fed_again_after_its_final_piece_starts_clean(hasher, mask, layout):
    """Final pieces with text, without text (the flag on an empty piece) and with
    an unfinished group to drop put both records back to their initial values;
    the same state arrays then take a second chunk from its first character."""
    chains = []
    for k, size in enumerate((T + 100, 2 * T + 1, 865, 58, 3)):
        d = W.chunk_bytes(size, seed=50 + k)
        t = ENCODE[layout](d)
        a = len(t) // 2 + k
        chains.append(Chain([t[:a], t[a:]], chunk=d, final_alone=k % 2 == 1, desc=f"{layout} {size} B"))
        cut = t[:len(t) - 4 - 2 - (3 if t.endswith(b"=") else 0)]  # ends two characters into a group: dropped
        chains.append(Chain([cut[:a], cut[a:]], desc=f"{layout} {size} B, an unfinished group at the end"))
    assert any(len(M.update(M.update(M.init(), c.pieces[0])[0], c.pieces[1])[0][1]) for c in chains)
    first = FlatFeed(chains, sphase=5, tphase=3, lines=mask[0], flat=mask[1])
    first.run(hasher)  # ends with both arrays as new_b64_states / new_states leave them
    again = FlatFeed(chains[::-1], sphase=3, tphase=5, lines=mask[0], flat=mask[1])
    again.b64, again.sha = first.b64, first.sha  # the records the first chunks' final pieces left
    again.run(hasher)

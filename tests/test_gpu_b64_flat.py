"""The flat path of the base64 decode on the GPU: unbroken RFC 4648 text, as
bitflood's Java and Perl peers frame a chunk (bitflood_amd/csrc/b64_flat.hip:
b64_flat_decode_kernel behind lbf_b64_verify_batch, b64_update_flat_kernel
between the line kernel and b64_update_kernel; lbf_set_b64_flat,
lbf_ctx_b64_flat_stats).

Expected values come from tests/wire_layouts.py and tests/wire_piece_model.py
(pinned to xmlrpc++'s recorded answers), tests/wire_flat_model.py and
tests/wire_line_model.py (held to those in tests/test_b64_flat_cpu.py and
tests/test_b64_lines_cpu.py) and hashlib, never from a GPU path.  Every
piecewise call is checked whole, as in tests/test_gpu_b64_update.py (whose Chain,
Feed and DeviceFeed run the rounds): both state arrays, every byte of the arena
-- 0xEE wherever nothing was decoded -- lengths, verdicts, and the counters.
Every one-shot call goes through tests/test_gpu_wire.py's _decode_and_check: a
0x5A-filled `out` with gaps between the slots and a stale-bytes call first.
"""
import numpy as np
import pytest

from bitflood_amd import B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, _capi, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import wire_flat_model as F
from tests import wire_layouts as W
from tests import wire_line_model as L
from tests import wire_piece_model as M
from tests.test_gpu_b64_lines import _period_chains
from tests.test_gpu_b64_update import FILL, Chain, DeviceFeed, Feed
from tests.test_gpu_wire import _decode_and_check

pytestmark = pytest.mark.gpu

T, TILE_TEXT = F.TILE_BYTES, F.TILE_TEXT
SIZES = (0, 1, 2, 3, 55, 57, 58, 864)
BIG = 5 * T + 1000


@pytest.fixture(autouse=True)
def flat_on():
    before = H.set_b64_flat(True)
    yield
    H.set_b64_flat(before)


@pytest.fixture(params=[True, False], ids=["lines", "no-lines"])
def lines(request):
    before = H.set_b64_lines(request.param)
    yield request.param
    H.set_b64_lines(before)


class FlatFeed(Feed):
    """Feed whose every call is also held to the counters.  The two paths'
    characters add up to the call's text and flat_chars is a share of
    scan_chars.  With the line path off the flat kernel reads the record itself
    and flat_chars is the model's tiled prefixes, to the character (no more than
    the longest flat prefixes: tests/test_b64_flat_cpu.py).  Behind the line
    kernel it is no more than the longest run of alphabet characters that starts
    where the line model's prefix may end, and of undamaged text the two take
    all but eight characters a piece.  With the switch off: nothing."""

    def __init__(self, chains, sphase=None, tphase=None, undamaged=True, lines=True, flat=True):
        super().__init__(chains, sphase, tphase)
        self.undamaged, self.lines, self.flat = undamaged, lines, flat
        self.flat_chars = 0

    def run_round(self, hasher, r, check_states=True):
        live = [k for k, c in enumerate(self.chains) if r < len(c.pieces)]
        total = most = exact = least = 0
        for k in live:
            piece, st = self.chains[k].pieces[r], self.model[k]
            total += len(piece)
            if not self.lines:
                exact += F.take(st, piece, tiles=True)[0]
            elif not st[2] and piece:
                most += F.most_behind_lines(L.take(st, piece)[0], piece)
                least += max(len(piece) - 8, 0)
        u0, f0 = hasher.b64_update_stats(), hasher.b64_flat_stats()
        res = super().run_round(hasher, r, check_states)
        u1, f1 = hasher.b64_update_stats(), hasher.b64_flat_stats()
        line, scan = u1["line_chars"] - u0["line_chars"], u1["scan_chars"] - u0["scan_chars"]
        flat = f1["flat_chars"] - f0["flat_chars"]
        assert line + scan == total, (r, line, scan, total)
        assert f1["flat_chunks"] == f0["flat_chunks"]
        assert flat <= scan, (r, flat, scan)
        if not self.flat:
            assert flat == 0, (r, flat)
        elif not self.lines:
            assert line == 0 and flat == exact, (r, line, flat, exact)
        else:
            assert flat <= most, (r, flat, most)
            if self.undamaged:
                assert line + flat >= least, (r, line, flat, least, total)
        self.flat_chars += flat
        return res


def big_text(seed=0):
    d = W.chunk_bytes(BIG, seed=seed)
    return d, F.text(d)


# ------------------------------------------------------------ 1. every cut of small unbroken texts
def _unbroken_chains():
    chains = []
    for n in SIZES:
        d = W.chunk_bytes(n)
        t = F.text(d)
        chains += [Chain([t[:a], t[a:]], chunk=d, desc=f"{n} B cut at {a}") for a in range(len(t) + 1)]
    assert all(c.verdict for c in chains)
    return chains


@pytest.mark.parametrize("sphase,tphase", [(0, 0), (0, 3), (5, 0), (5, 3)])
def test_every_cut_of_unbroken_texts(hasher, lines, sphase, tphase):
    """Less than one tile a piece: every carry, every output phase mod 16, both
    sides of the '=' group, pieces too short to complete a carried group."""
    feed = FlatFeed(_unbroken_chains(), sphase, tphase, lines=lines)
    feed.run(hasher)
    assert feed.flat_chars > 0


def test_every_cut_with_the_flat_path_off(hasher, lines):
    """The same feed with the switch off: the same bytes, records and verdicts
    (Feed checks them), and no character on the flat path."""
    assert H.set_b64_flat(False) is True
    FlatFeed(_unbroken_chains(), 5, 3, lines=lines, flat=False).run(hasher)
    assert H.set_b64_flat(True) is False


# ------------------------------------------------------------ 2. tile edges
def _edge_cuts(n):
    return sorted(set(range(0, 147)) | set(range(TILE_TEXT - 80, TILE_TEXT + 81)) | set(range(n - 160, n + 1)))


def test_two_piece_cuts_around_tile_edges(hasher, lines):
    """Five tiles and a part, cut at every character of the first 147, around
    the first tile edge and in the last 160 characters."""
    d, t = big_text()
    chains = [Chain([t[:a], t[a:]], chunk=d, desc=f"cut at {a}") for a in _edge_cuts(len(t))]
    firsts = [M.update(M.init(), t[:a])[0] for a in _edge_cuts(len(t)) if b"=" not in t[:a]]
    assert {len(carry) for _, carry, _ in firsts} == {0, 1, 2, 3}
    assert {dec % 16 for dec, _, _ in firsts} == set(range(16))
    feed = FlatFeed(chains, sphase=(0, 5)[lines], tphase=(3, 0)[lines], lines=lines)
    feed.run(hasher)
    assert feed.flat_chars > len(chains) * (len(t) - TILE_TEXT - 200)  # all but the line kernel's first tile


def test_tile_edge_cuts_through_the_device_resident_launch(lines):
    """lbf_b64_update_launch: the cuts around the first tile edge, three pieces
    a chain, everything in device buffers on a side stream."""
    d, t = big_text(seed=1)
    chains = [Chain([t[:a], t[a:a + TILE_TEXT + e], t[a + TILE_TEXT + e:]], chunk=d, desc=f"cuts at {a}, {e}")
              for a in (0, 1, 2, 3, 37) for e in range(-12, 13)]
    feed = Feed(chains, sphase=3 if lines else 12, tphase=9)
    text_max = max(feed.texts(range(len(chains)), r)[0].size for r in range(3))
    dev = DeviceFeed(feed, len(chains), text_max)
    try:
        for r in range(3):
            dev.run_round(r)
    finally:
        dev.close()
    assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()


# ------------------------------------------------------------ 3. damage stays unwritten on the device
HURT = ("space", "eq", "junk", "drop")


def hurt(t: bytes, kind: str, p: int) -> bytes:
    if kind == "space":
        return t[:p] + b" " + t[p + 1:]
    return W.damage(t, kind, p)


def _damage_places(n, lead=0):
    """The first group, both sides of the first two tile edges of the chunk
    (`lead` characters of it lie in front of this text), the last group."""
    ps = set(range(5))
    for edge in (TILE_TEXT - lead, 2 * TILE_TEXT - lead):
        ps.update(range(edge - 5, edge + 6))
    ps.update(range(n - 5, n))
    return sorted(p for p in ps if 0 <= p < n)


@pytest.mark.parametrize("kind", HURT)
def test_damage_stays_unwritten_on_the_device(hasher, lines, kind):
    """Device-resident, the arena read back whole after each launch: the
    model's bytes below the new `decoded`, 0xEE everywhere else -- in the slot
    past `decoded`, between slots, in the guards -- whatever a tile that held
    the damage had decoded before it showed.  Piece 2 starts with one sextet
    carried."""
    d, t = big_text(seed=2 + HURT.index(kind))
    first, rest = t[:101], t[101:]
    chains = [Chain([first, rest], chunk=d, desc="undamaged")]
    chains += [Chain([first, hurt(rest, kind, p)], cap=len(d), chunk=d, desc=f"{kind} at {p} of piece 2")
               for p in _damage_places(len(rest), lead=101)]
    feed = Feed(chains, sphase=9, tphase=6)
    text_max = max(feed.texts(range(len(chains)), r)[0].size for r in range(2))
    dev = DeviceFeed(feed, len(chains), text_max)
    try:
        dev.run_round(0)
        dev.run_round(1)
    finally:
        dev.close()
    assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()
    # the launch keeps no count; the batch call on the same inputs
    FlatFeed(chains, sphase=9, tphase=6, undamaged=False, lines=lines).run(hasher)


# ------------------------------------------------------------ 4. slot and length disagree
def test_slot_and_length_disagree_on_the_flat_path(hasher, lines):
    """A text of L bytes into slots of L - 1, L - 5, L - 17, L + 9 and one that
    ends inside the first block of a tile, as three pieces: nothing at or past
    cap (the guards behind every slot stay), out_sizes = cap + 1 and verdict 0
    where the text decodes to more, and the record counts on past the slot."""
    d, t = big_text(seed=7)
    n = len(d)
    chains = []
    for cap in (n - 1, n - 5, n - 17, n + 9, 2 * T + 7, n):
        for a, b in ((5000, 15000), (F.flat_len(cap // 3 * 3 - 300) if cap < n else 9000, len(t) - 50), (1, 74)):
            chains.append(Chain([t[:a], t[a:b], t[b:]], cap=cap, desc=f"cap {cap} of {n}, cuts at {a} and {b}"))
            assert chains[-1].size == (n if n <= cap else cap + 1) and chains[-1].verdict == (cap == n)
    feed = FlatFeed(chains, sphase=7, tphase=1, lines=lines)
    for r in range(feed.rounds):
        feed.run_round(hasher, r)
        feed.check_sha([r >= len(c.pieces) - 1 for c in feed.chains])
        for k, c in enumerate(feed.chains):
            if r < len(c.pieces) - 1:
                assert feed.b64["decoded"][k] == len(feed.sofar[k])
                assert feed.sha["total"][k] == min(len(feed.sofar[k]), c.cap)
    assert any(len(c.want) > c.cap for c in chains) and feed.flat_chars > 0


# ------------------------------------------------------------ 5. forged records
def test_forged_device_records_on_the_flat_path(lines):
    """Records the launch cannot read, forged, two tiles of unbroken text a
    piece, between guard bytes: ncarry = 255 and carry = all ones count & 3 and
    masked; `decoded` of 2^64 - 12, 2^64 - 1, 2^64 - 300, 2^61 and 7 are declined
    (clamped, they are no multiple of 3) and left to the general rule; 3 * 2^40
    is taken and writes nothing; a piece that names no chain is skipped and its
    work-array entries stay; a chunk over 1 GiB decodes nothing."""
    lib = _capi.load()
    cap, n_states = 9000, 10
    n = n_states + 1
    body = F.text(W.chunk_bytes(3 * T, seed=12))
    forged = [0, 96, 2**64 - 12, 2**64 - 1, 1 << 61, 7, 3 << 40, 0, 54, 2**64 - 300]
    carried = [True, True] + [False] * 8  # ncarry = 255, carry = 0xFFFFFFFF
    caps = np.full(n, cap, np.uint32)
    caps[7] = (1 << 30) + 1
    fin = np.array([0, 1, 0, 1, 0, 0, 0, 1, 0, 0, 1], np.uint8)
    b64, sha = new_b64_states(n_states + 1), new_states(n_states + 1)  # one guard record behind each array
    b64["decoded"][:n_states] = np.array(forged, dtype=np.uint64)
    b64["ncarry"][:n_states] = np.where(carried, 255, 0)
    b64["carry"][:n_states] = np.where(carried, 0xFFFFFFFF, 0)
    b64.view(np.uint8).reshape(-1, 16)[n_states] = FILL
    sha.view(np.uint8).reshape(-1, 96)[n_states] = FILL
    # what the kernels make of each record
    states = [(min(forged[k], 1 << 61), (63, 63, 63) if carried[k] else (), False) for k in range(n_states)]
    pieces = [body[k:k + 2 * TILE_TEXT + 1] for k in range(n)]
    assert all(F.take(states[k], pieces[k], tiles=True)[0] >= 2 * TILE_TEXT - 4 for k in (0, 1, 6, 8))
    assert all(F.take(states[k], pieces[k])[0] == 0 for k in (2, 3, 4, 5, 9))
    toff = np.cumsum([0] + [len(p) + 16 for p in pieces[:-1]]).astype(np.uint64)
    text = np.zeros(int(toff[-1]) + len(pieces[-1]) + 16, np.uint8)
    for k, p in enumerate(pieces):
        text[int(toff[k]):int(toff[k]) + len(p)] = np.frombuffer(p, np.uint8)
    slot = 64 + (cap + 240) * np.arange(n, dtype=np.uint64)
    out = np.full(64 + (cap + 240) * n, FILL, dtype=np.uint8)
    want_out = out.copy()
    want_b64 = new_b64_states(n_states)
    room, gain, sizes = [], [], []
    for k in range(n_states):
        if k == 7:  # over 1 GiB: nothing decoded; final, so the record is as new
            room.append(0)
            gain.append(0)
            sizes.append(0)
            continue
        after, new = M.update(states[k], pieces[k])
        lo, at = min(states[k][0], cap), int(slot[k])
        hi = min(states[k][0] + len(new), cap)
        room.append(cap - lo)
        gain.append(hi - lo if hi > lo else 0)
        total = states[k][0] + len(new)
        sizes.append(total if total <= cap else cap + 1)
        if hi > lo:
            want_out[at + lo:at + hi] = np.frombuffer(new[:hi - lo], np.uint8)
        if not fin[k]:
            want_b64[k] = M.b64_record((min(after[0], 1 << 61), after[1], after[2]))
    host = dict(b64=b64, sha=sha, so=np.arange(n, dtype=np.uint32), text=text, toff=toff,
                tlen=np.array([len(p) for p in pieces], np.uint32), fin=fin, out=out, ooff=slot, caps=caps,
                osz=np.full(n, 0xEEEEEEEE, np.uint32), dig=np.full(20 * n, FILL, np.uint8),
                exp=np.zeros(20 * n, np.uint8), ver=np.full(n, FILL, np.uint8),
                poff=np.full(n, 0xEEEEEEEEEEEEEEEE, np.uint64), psz=np.full(n, 0xEEEEEEEE, np.uint32))
    bufs = {k: DeviceBuffer(v.nbytes) for k, v in host.items()}
    try:
        for k, v in host.items():
            bufs[k].upload(v)
        H.b64_update_launch(bufs["b64"], bufs["sha"], n_states, bufs["so"], bufs["text"], bufs["toff"], bufs["tlen"],
                            bufs["fin"], n, bufs["out"], bufs["ooff"], bufs["caps"], bufs["osz"], bufs["dig"],
                            bufs["exp"], bufs["ver"], bufs["poff"], bufs["psz"])
        _capi.check(lib.lbf_device_synchronize())
        got = bufs["out"].download(out.size)
        wrong = np.flatnonzero(got != want_out)
        assert wrong.size == 0, (wrong[:8].tolist(), [int(x) for x in slot])
        psz = bufs["psz"].download(4 * n, dtype=np.uint32)
        poff = bufs["poff"].download(8 * n, dtype=np.uint64)
        assert psz[n_states] == 0xEEEEEEEE and poff[n_states] == 0xEEEEEEEEEEEEEEEE  # the skipped piece's entries
        for k in range(n_states):
            assert psz[k] == gain[k] <= room[k], (k, int(psz[k]), gain[k], room[k])  # never more than the slot has left
            if k != 7:
                assert poff[k] == int(slot[k]) + min(states[k][0], cap), k
        assert gain[8] == 2 * T and 0 < gain[0] < cap and gain[6] == 0 and gain[9] == 0
        b2 = bufs["b64"].download(b64.nbytes).view(B64_STATE_DTYPE)
        s2 = bufs["sha"].download(sha.nbytes).view(STATE_DTYPE)
        assert b2[n_states].tobytes() == bytes([FILL]) * 16 and s2[n_states].tobytes() == bytes([FILL]) * 96
        assert b2[:n_states].tobytes() == want_b64.tobytes(), (b2[:n_states], want_b64)
        assert b2["decoded"][[2, 4, 9]].tolist() == [1 << 61] * 3
        assert s2[[1, 3, 7]].tobytes() == new_states(3).tobytes()  # the final pieces' SHA records are as new
        osz, ver = bufs["osz"].download(4 * n, dtype=np.uint32), bufs["ver"].download(n)
        E = 0xEEEEEEEE
        assert osz.tolist() == [E, sizes[1], E, cap + 1, E, E, E, 0, E, E, E] and sizes[1] == 96 + gain[1]
        assert ver.tolist() == [FILL, 0, FILL, 0, FILL, FILL, FILL, 0, FILL, FILL, FILL]
    finally:
        for b in bufs.values():
            b.free()


# ------------------------------------------------------------ 6. ragged and corner cases
def _corner_chains(n, seed):
    rng = np.random.default_rng(seed)
    chains = []
    for i in range(n):
        size = int(rng.integers(0, 9001))
        d = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        t = F.text(d) if i % 4 else W.xmlrpc_text(d)  # a quarter in the encoder's layout: a mixed batch
        cuts = set(rng.integers(0, len(t) + 1, int(rng.integers(1, 5))).tolist())
        if i % 3 == 0 and len(t) > 9:  # a piece of one character
            at = int(rng.integers(0, len(t) - 1))
            cuts |= {at, at + 1}
        if i % 2 == 0 and t.endswith(b"="):  # a piece that holds only the "xx==" / "xxx=" group, or only '='
            cuts.add(len(t) - (4 if i % 4 else 1))
        cuts = [0] + sorted(cuts - {0, len(t)}) + [len(t)]
        pieces = [t[a:b] for a, b in zip(cuts, cuts[1:])]
        if i % 5 == 0:  # an empty piece in the middle
            pieces.insert(int(rng.integers(0, len(pieces) + 1)), b"")
        if i % 7 == 3 and t.endswith(b"="):  # text behind the end of the data: the chain has `ended` when it comes
            pieces.append(t[:146])
        chains.append(Chain(pieces, chunk=d, final_alone=i % 6 == 1, digest_ok=i % 11 != 0,
                            desc=f"chunk {i}: {size} B in {len(pieces)} pieces"))
        assert chains[-1].want == d and chains[-1].verdict == (i % 11 != 0)
    return chains


@pytest.mark.parametrize("n", [1, 64, 257])
def test_ragged_chains(hasher, lines, n):
    """Chunks of 0..9,000 bytes in one to eight pieces, unbroken and in the
    encoder's layout side by side, chains ending in different calls: empty
    pieces, pieces of one character, of the '=' group alone and of '=' alone,
    final pieces with and without text, text for a chain that has ended."""
    chains = _corner_chains(n, 9300 + n)
    if n >= 64:
        ps = [p for c in chains for p in c.pieces]
        assert b"" in ps and b"=" in ps and any(len(p) == 1 and p != b"=" for p in ps)
        assert any(len(p) == 4 and p.endswith(b"=") for p in ps)
    feed = FlatFeed(chains, sphase=(None if n % 2 else 11), tphase=(None if n > 64 else 5), lines=lines)
    feed.run(hasher)
    assert feed.flat_chars > 0 or n == 1  # chain 0 is in the encoder's layout


# ------------------------------------------------------------ 7. the encoder's layout with the switch on
def test_every_cut_of_16_line_texts_with_the_flat_path_on(hasher):
    """The line path's own feed: the same results, and behind the line kernel
    the flat kernel takes at most one line a piece."""
    chains = _period_chains()
    for c in chains:
        st = M.init()
        for p in c.pieces:
            assert F.most_behind_lines(L.take(st, p)[0], p) <= 72
            st, _ = M.update(st, p)
    before = H.set_b64_lines(True)
    try:
        FlatFeed(chains, 5, 3, lines=True).run(hasher)
    finally:
        H.set_b64_lines(before)


# ------------------------------------------------------------ 8. one-shot
def _one_shot(hasher, c, on=True):
    f0 = hasher.b64_flat_stats()
    res = _decode_and_check(hasher, c)
    f1 = hasher.b64_flat_stats()
    want = sum(F.decoded_flat(t, cap) for t, cap in zip(c.texts, c.caps))
    assert f1["flat_chunks"] - f0["flat_chunks"] == (want if on else 0)
    assert f1["flat_chars"] == f0["flat_chars"]
    return res, want


def _sizes_corpus():
    c = W.Corpus("flat/sizes")
    for size in (0, 1, 2, 3, 54, 55, 57, T - 1, T, T + 1, T + 3, BIG):
        d = W.chunk_bytes(size, seed=21)
        for tphase in range(16):
            for sphase in (0, 5, 11):
                c.add(F.text(d), d, f"{size} B text%16={tphase} slot%16={sphase}", tphase=tphase, sphase=sphase)
    return c


def test_one_shot_sizes_and_phases(hasher):
    """Unbroken texts on both sides of one tile and of the layouts' parting at
    55 bytes, at every text phase and three slot phases."""
    (ver, _, _), flat = _one_shot(hasher, _sizes_corpus())
    assert ver.all() and flat == 7 * 48


def test_one_shot_with_the_flat_path_off(hasher):
    """The switch off: the parent's route (one pass, then two), the same results."""
    assert H.set_b64_flat(False) is True
    try:
        (ver, _, _), _ = _one_shot(hasher, _sizes_corpus(), on=False)
    finally:
        H.set_b64_flat(True)
    assert ver.all()


@pytest.mark.parametrize("kind", HURT)
def test_one_shot_damage(hasher, kind):
    """Damage in the first group, on both sides of the tile edges and in the
    last group: what is not flat goes to the general kernel, with its bytes."""
    c = W.Corpus(f"flat/{kind}")
    for size in (T + 3, BIG, BIG + 1, BIG + 2):
        d = W.chunk_bytes(size, seed=22)
        t = F.text(d)
        c.add(t, d, f"{size} B undamaged", tphase=size % 16, sphase=5)
        for p in _damage_places(len(t)):
            c.add(hurt(t, kind, p), d, f"{size} B {kind} at {p}", tphase=p % 16, sphase=(0, 5, 11)[p % 3])
    (ver, _, want_ver), flat = _one_shot(hasher, c)
    # (an '=' put over an '=' and a dropped '=' leave the bytes as they were)
    assert 4 <= flat < len(c) and want_ver.sum() >= 4 and not want_ver.all()


def test_one_shot_slot_and_text_disagree_and_a_wrong_digest(hasher):
    """A text of L bytes for a slot of L - 1, L + 1, L - T and L + T bytes, L at
    every size mod 3 (a slot one byte off may or may not change the text's
    length), and one chunk whose expected digest is wrong."""
    c = W.Corpus("flat/disagree")
    stream = W.chunk_bytes(3 * T + 200, seed=23)
    for L_ in (2 * T + 100, 2 * T + 101, 2 * T + 102):
        for C in (L_, L_ - 1, L_ + 1, L_ - T, L_ + T):
            for sphase in (0, 5):
                c.add(F.text(stream[:L_]), stream[:C], f"L={L_} C={C} slot%16={sphase}", cap=C, tphase=3, sphase=sphase)
    c.add(F.text(stream[:T + 5]), stream[:T + 5], "wrong digest", digest_ok=False)
    (ver, dec, want_ver), flat = _one_shot(hasher, c)
    assert want_ver.sum() == 6 and 6 < flat < len(c)  # a candidate one byte off is decoded flat, and fails its length

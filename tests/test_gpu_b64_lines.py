"""The line path of the piecewise base64 decode on the GPU
(bitflood_amd/csrc/b64_update_lines.hip in front of b64_update_kernel;
lbf_set_b64_lines, lbf_ctx_b64_update_stats).

Expected values come from tests/wire_layouts.py and tests/wire_piece_model.py
(pinned to xmlrpc++'s recorded answers), tests/wire_line_model.py (held to
those in tests/test_b64_lines_cpu.py) and hashlib, never from a GPU path.
Every call is checked whole, as in tests/test_gpu_b64_update.py (whose Chain
and Feed run the rounds): both state arrays, every byte of the arena -- 0xEE
wherever nothing was decoded -- lengths and verdicts, and here the characters
the call sent down each path.
"""
import numpy as np
import pytest

from bitflood_amd import B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, _capi, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import wire_layouts as W
from tests import wire_line_model as L
from tests import wire_piece_model as M
from tests.test_gpu_b64_update import FILL, Chain, DeviceFeed, Feed, model_update

pytestmark = pytest.mark.gpu

TILE_TEXT, TILE_BYTES = W.DEC_TEXT, W.DEC_BYTES  # the line kernel's tile is the one-pass decode's


@pytest.fixture(autouse=True)
def lines_on():
    before = H.set_b64_lines(True)
    yield
    H.set_b64_lines(before)


class LineFeed(Feed):
    """Feed whose every call is also held to the stats: the two paths' characters
    add up to the call's text; the line path took no more than the model's
    prefixes and, of text that conforms, all but eight characters a piece."""

    def __init__(self, chains, sphase=None, tphase=None, conforming=True, lines=True):
        super().__init__(chains, sphase, tphase)
        self.conforming, self.lines = conforming, lines
        self.line_chars = 0

    def run_round(self, hasher, r, check_states=True):
        live = [k for k, c in enumerate(self.chains) if r < len(c.pieces)]
        total = most = least = 0
        for k in live:
            piece = self.chains[k].pieces[r]
            total += len(piece)
            most += L.take(self.model[k], piece)[0]
            if not self.model[k][2]:  # the text of a chain that has ended is the scan path's
                least += max(len(piece) - 8, 0)
        s0 = hasher.b64_update_stats()
        res = super().run_round(hasher, r, check_states)
        s1 = hasher.b64_update_stats()
        line, scan = s1["line_chars"] - s0["line_chars"], s1["scan_chars"] - s0["scan_chars"]
        assert line + scan == total, (r, line, scan, total)
        if not self.lines:
            assert line == 0, (r, line)
            return res
        assert line <= most, (r, line, most)
        if self.conforming:
            assert line >= least, (r, line, least, total)
        self.line_chars += line
        return res


def edge_text(k):
    d = W.chunk_bytes(W.EDGE_SIZES[k])
    return d, W.xmlrpc_text(d)


# ------------------------------------------------------------ 1. every cut of 16-line texts
def _period_chains():
    chains = []
    for n in W.PERIOD_SIZES:
        t = W.xmlrpc_text(W.chunk_bytes(n))
        chains += [Chain([t[:a], t[a:]], chunk=W.chunk_bytes(n), desc=f"{n} B cut at {a}") for a in range(len(t) + 1)]
    assert all(c.verdict for c in chains)
    return chains


@pytest.mark.parametrize("sphase,tphase", [(0, 0), (0, 3), (5, 0), (5, 3)])
def test_every_cut_of_16_line_texts(hasher, sphase, tphase):
    """Less than one tile a piece: the partial-tile path at every start column,
    carry and output phase, both sides of every separator and of the '=' group."""
    feed = LineFeed(_period_chains(), sphase, tphase)
    feed.run(hasher)
    assert feed.line_chars > 0


def test_every_cut_with_the_line_path_off(hasher):
    """The same feed through the general rule alone: the same bytes, records
    and verdicts (Feed checks them), and no character on the line path."""
    assert H.set_b64_lines(False) is True
    feed = LineFeed(_period_chains(), 5, 3, lines=False)
    feed.run(hasher)
    assert H.set_b64_lines(True) is False


# ------------------------------------------------------------ 2. tile edges, columns, output phases
@pytest.mark.parametrize("k", [0, 1])
def test_two_piece_cuts_around_tile_edges(hasher, k):
    """Five tiles and a part, cut at every character of the first two lines
    (every start column, every carry, every decoded mod 16 among them), around
    the first tile edge and in the last 160 characters."""
    d, t = edge_text(k)
    cuts = sorted(set(range(0, 147)) | set(range(TILE_TEXT - 80, TILE_TEXT + 81)) | set(range(len(t) - 160, len(t) + 1)))
    chains = [Chain([t[:a], t[a:]], chunk=d, desc=f"cut at {a}") for a in cuts]
    firsts = [model_update(M.init(), t[:a])[0] for a in cuts if b"=" not in t[:a]]
    assert {(4 * dec // 3 + len(carry)) % 72 for dec, carry, _ in firsts} == set(range(72))
    assert {dec % 16 for dec, _, _ in firsts} == set(range(16))
    LineFeed(chains, sphase=(0, 5)[k], tphase=(3, 0)[k]).run(hasher)


@pytest.mark.parametrize("a", [1, 37, 74, 2000])
def test_three_piece_cuts_around_one_and_two_tiles(hasher, a):
    """The middle piece is one or two tiles of text long, give or take 80
    characters: it ends on each side of a tile edge of the chunk, from a start
    inside a group, behind a separator, and mid-line."""
    d, t = edge_text(a % 2)
    chains = [Chain([t[:a], t[a:a + m + e], t[a + m + e:]], chunk=d, desc=f"cuts at {a} and {a + m + e}")
              for m in (TILE_TEXT, 2 * TILE_TEXT) for e in range(-80, 81)]
    LineFeed(chains, sphase=a % 16, tphase=(a // 3) % 16).run(hasher)


# ------------------------------------------------------------ 3. damage stays unwritten on the device
def _damage_places(n2):
    """Places in piece 2 (the text from character 100 on): its first group, the
    characters around the chunk's first and second tile edges, its last line."""
    ps = set(range(4))
    for edge in (TILE_TEXT - 100, 2 * TILE_TEXT - 100):
        ps.update(range(edge - 5, edge + 6))
    ps.update(range(n2 - 73, n2, 6))
    ps.update(range(n2 - 5, n2))
    return sorted(ps)


@pytest.mark.parametrize("kind", W.KINDS)
def test_damage_stays_unwritten_on_the_device(hasher, kind):
    """Device-resident, the arena read back whole after each launch: the
    model's bytes below the new `decoded`, 0xEE everywhere else -- in the slot
    past `decoded`, between slots, in the guards -- whatever a tile that broke
    the layout had decoded before its damage showed."""
    d, t = edge_text(W.KINDS.index(kind) % 2)
    first, rest = t[:100], t[100:]
    chains = [Chain([first, rest], chunk=d, desc="undamaged")]
    chains += [Chain([first, W.damage(rest, kind, p)], cap=len(d), chunk=d, desc=f"{kind} at {p} of piece 2")
               for p in _damage_places(len(rest))]
    feed = Feed(chains, sphase=9, tphase=6)
    text_max = max(feed.texts(range(len(chains)), r)[0].size for r in range(2))
    dev = DeviceFeed(feed, len(chains), text_max)
    try:
        dev.run_round(0)
        dev.run_round(1)
    finally:
        dev.close()
    assert feed.b64.tobytes() == new_b64_states(len(chains)).tobytes()
    # the launch keeps no count; the batch call on the same inputs: no more than the model's prefixes
    LineFeed(chains, sphase=9, tphase=6, conforming=False).run(hasher)


# ------------------------------------------------------------ 4. slot and length disagree
def test_slot_and_length_disagree_on_the_line_path(hasher):
    """A text of L bytes into slots of L - 1, L - 5, L - 17, L + 9 and one that
    ends inside the first block of a tile, as three pieces: nothing at or past
    cap (the guards behind every slot stay), out_sizes = cap + 1 and verdict 0
    where the text decodes to more, and the record counts on past the slot."""
    d, t = edge_text(1)
    n = len(d)
    chains = []
    for cap in (n - 1, n - 5, n - 17, n + 9, 2 * TILE_BYTES + 7, n):
        for a, b in ((5000, 15000), (W.b64_len(cap // 3 * 3 - 300) if cap < n else 9000, len(t) - 50), (1, 74)):
            chains.append(Chain([t[:a], t[a:b], t[b:]], cap=cap, desc=f"cap {cap} of {n}, cuts at {a} and {b}"))
            assert chains[-1].size == (n if n <= cap else cap + 1) and chains[-1].verdict == (cap == n)
    feed = LineFeed(chains, sphase=7, tphase=1)
    for r in range(feed.rounds):
        feed.run_round(hasher, r)
        feed.check_sha([r >= len(c.pieces) - 1 for c in feed.chains])
        for k, c in enumerate(feed.chains):
            if r < len(c.pieces) - 1:
                assert feed.b64["decoded"][k] == len(feed.sofar[k])
                assert feed.sha["total"][k] == min(len(feed.sofar[k]), c.cap)
    assert any(len(c.want) > c.cap for c in chains)


# ------------------------------------------------------------ 5. forged records
def test_forged_device_records_on_the_line_path():
    """test_forged_device_records_write_nothing_outside_slot_and_records with
    two tiles of text a piece that continues the layout from where the
    (clamped) record stands, so that the line kernel takes what it may: ncarry =
    255 and carry = all ones count & 3 and masked; `decoded` of 2^64 - 12,
    2^64 - 1, 2^61 and 7 are declined (clamped, they are no multiple of 3) and
    left to the general rule; a piece that names no chain is skipped and its
    work-array entries stay; a chunk over 1 GiB decodes nothing."""
    lib = _capi.load()
    cap, n_states = 9000, 9
    n = n_states + 1
    body = W.xmlrpc_text(W.chunk_bytes(3 * TILE_BYTES, seed=12))
    forged = [0, 96, 2**64 - 12, 2**64 - 1, 1 << 61, 7, 3 << 40, 0, 54]
    carried = [True, True, False, False, False, False, False, False, False]  # ncarry = 255, carry = 0xFFFFFFFF
    caps = np.full(n, cap, np.uint32)
    caps[7] = (1 << 30) + 1
    fin = np.array([0, 1, 0, 1, 0, 0, 0, 1, 0, 1], np.uint8)
    b64, sha = new_b64_states(n_states + 1), new_states(n_states + 1)  # one guard record behind each array
    b64["decoded"][:n_states] = np.array(forged, dtype=np.uint64)
    b64["ncarry"][:n_states] = np.where(carried, 255, 0)
    b64["carry"][:n_states] = np.where(carried, 0xFFFFFFFF, 0)
    b64.view(np.uint8).reshape(-1, 16)[n_states] = FILL
    sha.view(np.uint8).reshape(-1, 96)[n_states] = FILL
    # what the kernels make of each record, and the text that continues it
    states, pieces = [], []
    for k in range(n_states):
        dec = min(forged[k], 1 << 61)
        st = (dec, (63, 63, 63) if carried[k] else (), False)
        s = (4 * dec // 3 + len(st[1])) % 72 if dec % 3 == 0 else 0
        states.append(st)
        pieces.append(body[s:s + 2 * TILE_TEXT])
    pieces.append(pieces[0])
    assert all(L.take(states[k], pieces[k])[0] >= 2 * TILE_TEXT - 8 for k in (0, 1, 6, 8))
    assert all(L.take(states[k], pieces[k])[0] == 0 for k in (2, 3, 4, 5))
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
        assert gain[8] == 2 * TILE_BYTES and 0 < gain[0] < cap and gain[6] == 0
        b2 = bufs["b64"].download(b64.nbytes).view(B64_STATE_DTYPE)
        s2 = bufs["sha"].download(sha.nbytes).view(STATE_DTYPE)
        assert b2[n_states].tobytes() == bytes([FILL]) * 16 and s2[n_states].tobytes() == bytes([FILL]) * 96
        assert b2[:n_states].tobytes() == want_b64.tobytes(), (b2[:n_states], want_b64)
        assert b2["decoded"][[2, 4]].tolist() == [1 << 61, 1 << 61]
        assert s2[[1, 3, 7]].tobytes() == new_states(3).tobytes()  # the final pieces' SHA records are as new
        osz, ver = bufs["osz"].download(4 * n, dtype=np.uint32), bufs["ver"].download(n)
        E = 0xEEEEEEEE
        assert osz.tolist() == [E, sizes[1], E, cap + 1, E, E, E, 0, E, E] and sizes[1] == 96 + gain[1]
        assert ver.tolist() == [FILL, 0, FILL, 0, FILL, FILL, FILL, 0, FILL, FILL]
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
        t = W.xmlrpc_text(d)
        cuts = set(rng.integers(0, len(t) + 1, int(rng.integers(1, 5))).tolist())
        if i % 3 == 0 and len(t) > 73:  # a piece that holds only a separator
            line = int(rng.integers(0, len(t) // 73))
            cuts |= {73 * line + 72, 73 * line + 73}
        if i % 4 == 0 and t.endswith(b"="):  # a piece that holds only the "xx==" / "xxx=" group
            cuts.add(len(t) - 4)
        cuts = [0] + sorted(cuts - {0, len(t)}) + [len(t)]
        pieces = [t[a:b] for a, b in zip(cuts, cuts[1:])]
        if i % 5 == 0:  # an empty piece in the middle
            pieces.insert(int(rng.integers(0, len(pieces) + 1)), b"")
        if i % 7 == 3 and t.endswith(b"="):  # text behind the end of the data: the chain has `ended` when it comes
            pieces.append(b" " + t[:146])
        chains.append(Chain(pieces, chunk=d, final_alone=i % 6 == 1, digest_ok=i % 11 != 0,
                            desc=f"chunk {i}: {size} B in {len(pieces)} pieces"))
        assert chains[-1].want == d and chains[-1].verdict == (i % 11 != 0)
    return chains


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged_conforming_chains(hasher, n):
    """Chunks of 0..9,000 bytes in one to eight pieces, chains ending in
    different calls: empty pieces, pieces of a separator alone and of the '='
    group alone, final pieces with and without text, text for a chain that has
    ended."""
    chains = _corner_chains(n, 9100 + n)
    if n >= 63:
        assert any(b"" in c.pieces[:-1] for c in chains) and any(b" " in c.pieces for c in chains)
        assert any(len(p) == 4 and p.endswith(b"=") for c in chains for p in c.pieces)
        assert any(c.pieces[-1] == b"" for c in chains) and any(c.pieces[-1].startswith(b" ") for c in chains)
    LineFeed(chains, sphase=(None if n % 2 else 11), tphase=(None if n > 64 else 5)).run(hasher)

"""Chunks' base64 text decoded and hashed piece by piece on the GPU: resumable
decoder states beside the resumable SHA-1 states (lbf_b64_state,
lbf_b64_update_batch / lbf_b64_update_launch, ChunkHasher.update_text,
libBitFlood::PieceHasher::UpdateText).

Expected values never come from a GPU path: bytes and lengths from
tests/wire_layouts.decode / b64get (pinned to xmlrpc++'s recorded answers),
digests from hashlib, the states after a piece that is not the last from
tests/wire_piece_model.py and tests/sha1_model.py (pinned in
tests/test_b64_update_cpu.py and tests/test_update_cpu.py).  Every call is
checked whole: both state arrays, every byte of the output arena -- the bytes
decoded so far where they belong, 0xEE everywhere else, so nothing is
zero-filled and nothing outside a slot is touched -- lengths and verdicts.
"""
import ctypes
import functools
import hashlib
import itertools
import os
import subprocess

import numpy as np
import pytest

from bitflood_amd import (B64_STATE_DTYPE, STATE_DTYPE, ChunkHasher, DeviceBuffer, LbfError, _capi, new_b64_states,
                          new_states)
from bitflood_amd import hashing as H
from tests import wire_layouts as W
from tests import wire_piece_model as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xEE


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


@functools.lru_cache(maxsize=None)
def reference(text: bytes) -> bytes:
    return W.decode(text)


@functools.lru_cache(maxsize=None)
def model_update(state, piece: bytes):
    return M.update(state, piece)


class Chain:
    """One chunk's text as the pieces it arrives in.  `cap` is the size the
    receiver expects (default: what the text decodes to); `chunk` the bytes it
    expects (default: the decoded bytes below cap, so that only the length can
    fail the verdict); final_alone puts the final flag on an extra, empty piece."""

    def __init__(self, pieces, cap=None, chunk=None, digest_ok=True, final_alone=False, desc=""):
        self.pieces = [bytes(p) for p in pieces] + ([b""] if final_alone else [])
        self.want = reference(b"".join(self.pieces))
        self.cap = len(self.want) if cap is None else cap
        digest = sha1(self.want[:self.cap] if chunk is None else chunk)
        self.verdict = digest_ok and len(self.want) == self.cap and sha1(self.want) == digest
        self.expected = digest if digest_ok else bytes([digest[0] ^ 0x40]) + digest[1:]
        self.size = len(self.want) if len(self.want) <= self.cap else self.cap + 1
        self.desc = desc


class Feed:
    """Chains fed round by round through update_text (piece r of every chain
    that has one goes in call r), everything checked after every call."""

    def __init__(self, chains, sphase=None, tphase=None):
        self.chains, self.tphase = chains, tphase
        n = len(chains)
        self.caps = np.array([c.cap for c in chains], dtype=np.uint32)
        # slots touch (sphase None), or start at sphase mod 16 with guard bytes between
        self.slot = np.zeros(n, dtype=np.uint64)
        pos = 16
        for k, c in enumerate(chains):
            if sphase is not None:
                pos = (pos + 1 + 15) // 16 * 16 + sphase
            self.slot[k] = pos
            pos += c.cap
        self.out = np.full(pos + 16, FILL, dtype=np.uint8)
        self.want_out = self.out.copy()
        self.b64, self.sha = new_b64_states(n), new_states(n)
        self.model = [M.init()] * n
        self.sofar = [b""] * n
        self.expected = np.frombuffer(b"".join(c.expected for c in chains), dtype=np.uint8).reshape(n, 20)
        self.rounds = max(len(c.pieces) for c in chains)

    def texts(self, live, r):
        """The round's pieces in one buffer: one after another, or each at tphase mod 16."""
        parts, offs, pos = [], [], 0
        for k in live:
            p = self.chains[k].pieces[r]
            pad = 0 if self.tphase is None else (self.tphase - pos) % 16
            parts.append(bytes(pad) + p)
            offs.append(pos + pad)
            pos += pad + len(p)
        return np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8), offs

    def run_round(self, hasher, r, check_states=True):
        live = [k for k, c in enumerate(self.chains) if r < len(c.pieces)]
        fin = [r == len(self.chains[k].pieces) - 1 for k in live]
        text, offs = self.texts(live, r)
        sizes, ver = hasher.update_text(self.b64, self.sha, text, offs, [len(self.chains[k].pieces[r]) for k in live],
                                        self.out, self.slot[live], self.caps[live], state_of=live, final=fin,
                                        expected=self.expected[live])
        bad = []
        for j, k in enumerate(live):
            c = self.chains[k]
            before = len(self.sofar[k])
            if fin[j]:
                self.model[k], self.sofar[k] = M.init(), c.want  # Final() restarts the chain
                if sizes[j] != c.size or bool(ver[j]) != c.verdict:
                    bad.append((k, c.desc, "final", int(sizes[j]), c.size, bool(ver[j]), c.verdict))
            else:
                self.model[k], new = model_update(self.model[k], c.pieces[r])
                self.sofar[k] += new
                if sizes[j] != 0 or ver[j]:
                    bad.append((k, c.desc, "not final", int(sizes[j]), bool(ver[j])))
            s, lo, hi = int(self.slot[k]), min(before, c.cap), min(len(self.sofar[k]), c.cap)
            self.want_out[s + lo:s + hi] = np.frombuffer(self.sofar[k][lo:hi], dtype=np.uint8)
        assert not bad, bad[:5]
        wrong = np.flatnonzero(self.out != self.want_out)
        assert wrong.size == 0, (wrong[:8].tolist(), self.where(int(wrong[0])))
        if check_states:
            want_b64 = M.b64_records(self.model, B64_STATE_DTYPE)
            diff = np.flatnonzero(self.b64.view(np.uint8).reshape(-1, 16) != want_b64.view(np.uint8).reshape(-1, 16))
            assert diff.size == 0, (self.chains[int(diff[0]) // 16].desc, self.b64[int(diff[0]) // 16],
                                    want_b64[int(diff[0]) // 16])
        return sizes, ver

    def check_sha(self, final_round_done):
        """The SHA records: a chain that has ended is fresh again; one under way
        has absorbed what lies below its cap."""
        states = []
        for k, c in enumerate(self.chains):
            done = final_round_done[k]
            states.append(M.sha_state(b"" if done else self.sofar[k], c.cap))
        want = M.sha_records(states, STATE_DTYPE)
        bad = M.sha_records_differ(self.sha, want)
        assert not bad, [(k, self.chains[k].desc, self.sha[k], want[k]) for k in bad[:3]]
        ended = [k for k in range(len(self.chains)) if final_round_done[k]]
        assert self.sha[ended].tobytes() == new_states(len(ended)).tobytes()

    def where(self, at):
        k = int(np.searchsorted(self.slot, at, side="right")) - 1
        return f"byte {at}: slot {k} ({self.chains[k].desc}) + {at - int(self.slot[k])}, cap {self.chains[k].cap}"

    def run(self, hasher, check_states=True):
        for r in range(self.rounds):
            self.run_round(hasher, r, check_states)
            if check_states:
                self.check_sha([r >= len(c.pieces) - 1 for c in self.chains])
        assert self.b64.tobytes() == new_b64_states(len(self.chains)).tobytes()
        assert self.sha.tobytes() == new_states(len(self.chains)).tobytes()


# ------------------------------------------------------------ 1. every cut position
@pytest.mark.parametrize("sphase,tphase", [(0, 0), (0, 3), (5, 0), (5, 3)])
def test_every_cut_position(hasher, sphase, tphase):
    """The undamaged 16-line texts cut in two at every character, one chain per
    cut: after piece 1 both state arrays are the model's and the slot holds the
    decode's prefix; after the final piece bytes, lengths, verdict 1 and both
    records as new."""
    chains = []
    for n in W.PERIOD_SIZES:
        t = W.xmlrpc_text(W.chunk_bytes(n))
        assert reference(t) == W.chunk_bytes(n)
        chains += [Chain([t[:a], t[a:]], chunk=W.chunk_bytes(n), desc=f"{n} B cut at {a}") for a in range(len(t) + 1)]
    assert all(c.verdict for c in chains)
    Feed(chains, sphase, tphase).run(hasher)


# ------------------------------------------------------------ 2. tiny alphabet, exhaustive
def test_tiny_alphabet_every_text_every_cut(hasher):
    """All 5,461 texts of length <= 6 over A Q = * at every 2-way cut: '='
    completing a carried group at every ncarry, '=' in a group's first two
    places, text after the end of the data, junk-only pieces, an unfinished
    group dropped at the end.  Bytes and lengths are b64get's."""
    chains = []
    for n in range(7):
        for t in itertools.product(b"AQ=*", repeat=n):
            t = bytes(t)
            want = W.b64get(t)
            assert reference(t) == want
            chains += [Chain([t[:a], t[a:]], desc=f"{t!r} cut at {a}") for a in range(n + 1)]
    assert len(chains) == 36409
    carried = {(len(model_update(M.init(), c.pieces[0])[0][1]), c.pieces[1][:1]) for c in chains}
    assert {(nc, b"=") for nc in range(4)} <= carried
    Feed(chains).run(hasher)


# ------------------------------------------------------------ 3. damage next to a cut
@pytest.mark.parametrize("kind", W.KINDS)
def test_damage_next_to_a_cut(hasher, kind):
    """period_corpus(kind) at every 7th position, each text cut two characters
    before the damage, at it, and up to two behind it."""
    corpus = W.period_corpus(kind, step=7)
    places = []
    for n in W.PERIOD_SIZES:
        t = W.xmlrpc_text(W.chunk_bytes(n))
        places += [None] + list(W.positions(len(t), kind)[::7])
    assert len(places) == len(corpus)
    chains = []
    for t, d, p, desc in zip(corpus.texts, corpus.chunks, places, corpus.desc):
        for a in ([len(t) // 2] if p is None else sorted({min(max(p + k, 0), len(t)) for k in range(-2, 3)})):
            chains.append(Chain([t[:a], t[a:]], cap=len(d), chunk=d, desc=f"{desc} cut at {a}"))
    # the undamaged texts verify; the damaged ones do not, but for junk put between the characters
    assert any(c.verdict for c in chains) and (kind == "ins_junk") == all(c.verdict for c in chains)
    Feed(chains, sphase=(3 if kind in ("eq", "drop") else None)).run(hasher)


# ------------------------------------------------------------ 4. trip edges with a carry
def _cut_with_carry(t: bytes, near: int, nc: int) -> int:
    """The first cut at or behind `near` that leaves nc sextets pending."""
    a = near
    while len(model_update(M.init(), t[:a])[0][1]) != nc or model_update(M.init(), t[:a])[0][2]:
        a += 1
    return a


@pytest.mark.parametrize("nc", [0, 1, 2, 3])
def test_trip_edges_damage_with_a_carry(hasher, nc):
    """A seven-trip text cut so that piece 2 starts with nc sextets pending
    (the trips' sextets then sit nc places further on in the buffer); every kind
    of damage 17 characters to both sides of trips 1, 2 and 5 of piece 2, and a
    junk run longer than two trips inside piece 1, inside piece 2, and across
    the cut."""
    n = W.EDGE_SIZES[nc % 2]
    d = W.chunk_bytes(n)
    t = W.xmlrpc_text(d)
    a = _cut_with_carry(t, 4000 + 37 * nc, nc)
    first, rest = t[:a], t[a:]
    assert len(rest) > 5 * W.SCAN_CHARS + 100
    chains = [Chain([first, rest], chunk=d, desc="undamaged")]
    for kind in W.KINDS:
        for k in (1, 2, 5):
            for off in (-17, 17):
                p = W.SCAN_CHARS * k + off
                chains.append(Chain([first, W.damage(rest, kind, p)], cap=n, chunk=d,
                                    desc=f"{kind} at {p} of piece 2"))
    run = bytes(W.JUNK[k % len(W.JUNK)] for k in range(2 * W.SCAN_CHARS + 9))
    chains.append(Chain([first[:1500] + run + first[1500:], rest], chunk=d, desc="junk run in piece 1"))
    chains.append(Chain([first, rest[:5000] + run + rest[5000:]], chunk=d, desc="junk run in piece 2"))
    chains.append(Chain([first + run[:4100], run[4100:] + rest], chunk=d, desc="junk run across the cut"))
    chains.append(Chain([first, run, rest], chunk=d, desc="a piece of junk alone"))
    assert sum(c.verdict for c in chains) >= 5
    Feed(chains, sphase=nc, tphase=(0, 3, None, 7)[nc]).run(hasher)


def test_trip_edges_first_eq_with_a_carry(hasher):
    """The first '=' of piece 2 at character 4096k + j - ncarry, j = -5..5: its
    sextet index in the trip buffer runs through every place around a trip's
    end, after every carry.  More '=' behind it, and junk-free text so that
    character and sextet places agree."""
    chains = []
    for nc in range(4):
        first = W._alpha_stream(400 + nc, 40 + nc)
        for k in (1, 2):
            for j in range(-5, 6):
                q = W.SCAN_CHARS * k + j - nc
                t = bytearray(W._alpha_stream(q + 1 + 4200, 200 + 16 * k + j + 100 * nc))
                t[q] = ord("=")
                for later in (q + 1, q + 700, len(t) - 1):
                    if later != q + 1 or j % 2:
                        t[later] = ord("=")
                chains.append(Chain([first, bytes(t)], desc=f"ncarry {nc}, first '=' at {q} of piece 2"))
    assert {len(c.want) % 3 for c in chains} == {0, 1, 2}
    Feed(chains, sphase=1, tphase=2).run(hasher)


# ------------------------------------------------------------ 5. SHA corners through text
@pytest.mark.parametrize("final_alone", [False, True])
def test_sha_corners_through_text(hasher, final_alone):
    """Piece 1 decodes to 0, 3, 54, 57, 63, 66, 126 or 129 bytes and the chunk
    to 55..128: the update kernel meets every buffered x size corner around the
    64-byte block and the 56-byte padding edge with bytes the decode just wrote."""
    chains = []
    for total in (55, 56, 63, 64, 65, 119, 120, 128):
        d = W.chunk_bytes(total, seed=9)
        t = W.xmlrpc_text(d)
        for first in (0, 3, 54, 57, 63, 66, 126, 129):
            if first > total // 3 * 3:
                continue
            # the cut behind the group that completes `first` bytes, plus 0..3 characters of the next one
            a = min(W.b64_len(first) + (first + total) % 4, len(t))
            while b"=" in t[:a]:
                a -= 1
            c = Chain([t[:a], t[a:]], chunk=d, final_alone=final_alone, desc=f"{first} of {total} B, cut at {a}")
            assert len(model_update(M.init(), c.pieces[0])[1]) == first, c.desc
            chains.append(c)
    assert len(chains) >= 40 and all(c.verdict for c in chains)
    Feed(chains, sphase=0).run(hasher)


# ------------------------------------------------------------ 6. ragged
def _ragged_chains(n, seed):
    rng = np.random.default_rng(seed)
    chains = []
    for i in range(n):
        d = rng.integers(0, 256, int(rng.integers(0, 5001)), dtype=np.uint8).tobytes()
        t = W.xmlrpc_text(d)
        if i % 7 == 0:
            t = W.damage(t, "ins_junk", int(rng.integers(0, len(t) + 1)))
        cuts = [0] + sorted(rng.integers(0, len(t) + 1, int(rng.integers(2, 8))).tolist()) + [len(t)]
        chains.append(Chain([t[a:b] for a, b in zip(cuts, cuts[1:])], chunk=d, digest_ok=i % 11 != 0,
                            desc=f"chunk {i}: {len(d)} B in {len(cuts) - 1} pieces"))
        assert chains[-1].want == d and chains[-1].verdict == (i % 11 != 0)
    return chains


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_ragged(hasher, n):
    """Chunks of 0..5,000 bytes fed in three to eight random cuts through
    state_of, chains ending in different calls; every 7th text has junk
    inserted (bytes and verdict still right), every 11th expected digest is
    wrong (verdict 0, bytes still right)."""
    Feed(_ragged_chains(n, 8000 + n), sphase=(None if n % 2 else 11), tphase=(None if n > 64 else 5)).run(hasher)


# ------------------------------------------------------------ 7. slot and length disagree
def test_slot_and_length_disagree(hasher):
    """Texts that decode to cap - 1, cap + 1 and cap + 5 bytes, the excess
    arriving in a later piece: the slot gets its cap bytes and no more, the
    guard bytes around it stay, out_sizes = cap + 1, verdict 0 although the
    digest of the slot's bytes is the expected one, and the SHA record stops at
    cap while the decoder counts on."""
    chains = []
    for cap in (0, 1, 2, 3, 63, 64, 65, 300, 4097):
        for delta in (-1, 0, 1, 5):
            if cap + delta < 0:
                continue
            d = W.chunk_bytes(cap + delta, seed=4)
            t = W.xmlrpc_text(d)
            a = W.b64_len(cap // 3 * 3)  # the groups that fit the slot whole; the rest comes later
            for pieces in ([t[:a], t[a:]], [t[:a], t[a:a + 2], t[a + 2:], b""], [t]):
                chains.append(Chain(pieces, cap=cap, desc=f"cap {cap}, text decodes to {cap + delta}"))
                assert chains[-1].verdict == (delta == 0)
                assert chains[-1].size == (cap + delta if delta <= 0 else cap + 1)
    feed = Feed(chains, sphase=7, tphase=1)
    for r in range(feed.rounds):
        feed.run_round(hasher, r)
        feed.check_sha([r >= len(c.pieces) - 1 for c in feed.chains])
        for k, c in enumerate(feed.chains):
            if r < len(c.pieces) - 1:  # under way: the decoder's true count against the hash's capped one
                assert feed.b64["decoded"][k] == len(feed.sofar[k])
                assert feed.sha["total"][k] == min(len(feed.sofar[k]), c.cap)
    assert any(len(c.want) > c.cap and len(c.pieces) == 4 for c in chains)


# ------------------------------------------------------------ 8. refusals
def _raw_update_text(hasher, b64, sha, text, toff, tlen, fin, esz, exp, out, ooff, sizes, ver, state_of=None):
    a = lambda x, dt: None if x is None else np.ascontiguousarray(x, dtype=dt)  # noqa: E731
    toff, tlen, esz, ooff, so, fin = (a(toff, np.uint64), a(tlen, np.uint32), a(esz, np.uint32), a(ooff, np.uint64),
                                      a(state_of, np.uint32), a(fin, np.uint8))
    p = lambda x: None if x is None else x.ctypes.data  # noqa: E731
    return _capi.load().lbf_b64_update_batch(hasher._h, b64.ctypes.data, sha.ctypes.data, b64.size, p(so),
                                             text.ctypes.data, text.size, p(toff), p(tlen), p(fin), toff.size, p(esz),
                                             p(exp), p(out), out.size, p(ooff), p(sizes), p(ver))


def test_refusals_leave_states_and_outputs_untouched(hasher):
    d = [W.chunk_bytes(200, seed=k) for k in range(4)]
    texts = [W.xmlrpc_text(x) for x in d]
    text = np.frombuffer(b"".join(texts) + b"\0", dtype=np.uint8)
    toff = np.cumsum([0] + [len(t) for t in texts[:-1]])
    b64, sha = new_b64_states(4), new_states(4)
    out = np.full(1000, FILL, dtype=np.uint8)
    ooff = np.array([0, 200, 400, 600])
    caps = np.array([200, 200, 200, 200])
    # every chain mid-chunk: 30, 60, 92 and 123 characters in
    hasher.update_text(b64, sha, text, toff, [30, 60, 92, 123], out, ooff, caps)
    assert b64["ncarry"].tolist() == [2, 0, 3, 2] and (b64["decoded"] > 0).all()

    def forged(field, value, sha_total=None, **more):
        b, s = b64.copy(), sha.copy()
        for f, v in {field: value, **more}.items():
            b[f][1] = v
        if sha_total is not None:
            s["total"][1], s["buffered"][1] = sha_total, sha_total % 64
        return b, s

    ended = forged("ended", 1)
    ended[0]["decoded"][1] += 1  # fine once the data has ended ...
    ended[1]["total"][1] += 1
    ended[1]["buffered"][1] += 1
    ended[1]["block"][1][ended[1]["buffered"][1] - 1] = 0
    tl, one = [10, 10, 10], [200, 200, 200]
    cases = [
        ("ncarry", *forged("ncarry", 4), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("carry", *forged("carry", 1), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("carry", *forged("carry", 1 << 12, ncarry=2), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("ended", *forged("ended", 2), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("zero", *forged("zero", 1), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("multiple of 3", *forged("decoded", 46, 46), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("2^61", *forged("decoded", 3 << 60, 200), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("SHA state total", *forged("decoded", 48, 45), toff[:3], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("SHA state total", b64, sha, toff[:3], tl, ooff[:3], [200, 40, 200], [0, 1, 2], 1000),
        ("second piece", b64, sha, toff[:3], tl, ooff[:3], one, [2, 0, 2], 1000),
        ("text outside", b64, sha, [0, text.size - 5, 50], tl, ooff[:3], one, [0, 1, 2], 1000),
        ("slot outside", b64, sha, toff[:3], tl, [0, 801, 400], one, [0, 1, 2], 1000),
        ("slot outside", b64, sha, toff[:3], tl, ooff[:3], one, [0, 1, 2], 399),
        ("names state 4", b64, sha, toff[:3], tl, ooff[:3], one, [0, 4, 2], 1000),
        ("overlaps", b64, sha, toff[:3], tl, [0, 199, 400], one, [0, 1, 2], 1000),
        ("1 GiB", b64, sha, toff[:3], tl, ooff[:3], [200, (1 << 30) + 1, 200], [0, 1, 2], 1000),
    ]
    for what, b, s, to, tlens, oo, cp, so, out_len in cases:
        b, s = b.copy(), s.copy()
        before = b.tobytes(), s.tobytes(), out.tobytes()
        sizes = np.full(3, 0xEEEEEEEE, dtype=np.uint32)
        ver = np.full(3, FILL, dtype=np.uint8)
        rc = _raw_update_text(hasher, b, s, text, to, tlens, np.ones(3), cp, np.zeros((3, 20), np.uint8), out[:out_len],
                              oo, sizes, ver, state_of=so)
        msg = _capi.load().lbf_last_error().decode()
        piece = "piece 2 " if what == "second piece" else "piece 1 "
        assert rc == _capi.LBF_ERR_INVALID and what in msg and piece in msg, (what, rc, msg)
        assert (b.tobytes(), s.tobytes(), out.tobytes()) == before, what
        assert (sizes == 0xEEEEEEEE).all() and (ver == FILL).all(), what
    with pytest.raises(LbfError):
        hasher.update_text(b64, sha, text, [0, 0], [1, 1], out, [0, 200], [200, 200], state_of=[1, 1])
    # a record whose data has ended on any count passes, and the context still works
    rest = [len(t) - k for t, k in zip(texts, [30, 60, 92, 123])]
    exp = np.frombuffer(b"".join(sha1(x) for x in d), dtype=np.uint8).reshape(4, 20)
    sizes, ver = hasher.update_text(ended[0], ended[1], text, toff + [30, 60, 92, 123], rest, out, ooff, caps,
                                    final=np.ones(4), expected=exp)
    assert ver.tolist() == [True, False, True, True] and sizes[[0, 2, 3]].tolist() == [200, 200, 200]
    for k in (0, 2, 3):
        assert out[200 * k:200 * k + 200].tobytes() == d[k]
    assert (out[800:] == FILL).all()


# ------------------------------------------------------------ 9. states travel
def test_states_travel_as_bytes():
    chains = _ragged_chains(70, 99)
    two = [Chain([c.pieces[0], b"".join(c.pieces[1:])], chunk=c.want, desc=c.desc) for c in chains]
    feed = Feed(two, sphase=2)
    with ChunkHasher(device_mask=1) as h1:
        feed.run_round(h1, 0)
    stored = feed.b64.tobytes(), feed.sha.tobytes()
    assert len(stored[0]) == 16 * 70 and len(stored[1]) == 96 * 70
    feed.b64 = np.frombuffer(stored[0], dtype=B64_STATE_DTYPE).copy()
    feed.sha = np.frombuffer(stored[1], dtype=STATE_DTYPE).copy()
    with ChunkHasher(device_mask=1) as h2:
        feed.run_round(h2, 1)
    assert feed.b64.tobytes() == new_b64_states(70).tobytes() and feed.sha.tobytes() == new_states(70).tobytes()


# ------------------------------------------------------------ 10. launch cutting
def test_piece_larger_than_a_launch_is_cut(monkeypatch):
    """LBF_UPDATE_MB=1: a 3 MiB piece of text (a junk character in front, so
    the cuts fall inside groups) runs as several launches; bytes, length and
    verdict are those of the uncut call, and a second chain rides along."""
    d = W.chunk_bytes(2340000, seed=1)
    t = b"*" + W.xmlrpc_text(d)
    assert len(t) > 3 << 20
    small = W.xmlrpc_text(W.chunk_bytes(1000, seed=2))
    results = []
    for mb in ("1", "256"):
        monkeypatch.setenv("LBF_UPDATE_MB", mb)
        feed = Feed([Chain([t[:1001], t[1001:]], chunk=d, desc="3 MiB"), Chain([small[:7], small[7:]], desc="small")],
                    sphase=0, tphase=1)
        with ChunkHasher(device_mask=1) as h:
            feed.run_round(h, 0)
            results.append(feed.run_round(h, 1, check_states=False))
        assert feed.out[int(feed.slot[0]):int(feed.slot[0]) + len(d)].tobytes() == d
        assert feed.b64.tobytes() == new_b64_states(2).tobytes() and feed.sha.tobytes() == new_states(2).tobytes()
    assert results[0][0].tolist() == results[1][0].tolist() == [len(d), 1000]
    assert results[0][1].tolist() == results[1][1].tolist() == [True, True]


# ------------------------------------------------------------ 11. device-resident
class DeviceFeed:
    """Feed's rounds through b64_update_launch: everything in DeviceBuffers, on a side stream."""

    NAMES = ("b64", "sha", "so", "text", "toff", "tlen", "fin", "out", "ooff", "caps", "osz", "dig", "exp", "ver",
             "poff", "psz")

    def __init__(self, feed: Feed, n_max, text_max):
        self.feed, n = feed, len(feed.chains)
        size = dict(b64=16 * n, sha=96 * n, so=4 * n_max, text=text_max, toff=8 * n_max, tlen=4 * n_max, fin=n_max,
                    out=feed.out.size, ooff=8 * n_max, caps=4 * n_max, osz=4 * n_max, dig=20 * n_max, exp=20 * n_max,
                    ver=n_max, poff=8 * n_max, psz=4 * n_max)
        self.n_max = n_max
        self.bufs = {k: DeviceBuffer(v) for k, v in size.items()}
        self.stream = ctypes.c_void_p()
        _capi.check(_capi.load().lbf_stream_create(ctypes.byref(self.stream)))
        self.bufs["b64"].upload(feed.b64)
        self.bufs["sha"].upload(feed.sha)
        self.bufs["out"].upload(feed.out)

    def close(self):
        for b in self.bufs.values():
            b.free()
        _capi.check(_capi.load().lbf_stream_destroy(self.stream))

    def args(self, m, **swap):
        b = {**self.bufs, **swap}
        return (b["b64"], b["sha"], len(self.feed.chains), b["so"], b["text"], b["toff"], b["tlen"], b["fin"], m,
                b["out"], b["ooff"], b["caps"], b["osz"], b["dig"], b["exp"], b["ver"], b["poff"], b["psz"])

    def upload_round(self, r):
        f = self.feed
        live = [k for k, c in enumerate(f.chains) if r < len(c.pieces)]
        fin = np.array([r == len(f.chains[k].pieces) - 1 for k in live], dtype=np.uint8)
        text, offs = f.texts(live, r)
        up = dict(so=np.array(live, dtype=np.uint32), text=text, toff=np.array(offs, dtype=np.uint64),
                  tlen=np.array([len(f.chains[k].pieces[r]) for k in live], dtype=np.uint32), fin=fin,
                  ooff=f.slot[live], caps=f.caps[live], exp=f.expected[live],
                  osz=np.full(len(live), 0xEEEEEEEE, dtype=np.uint32), ver=np.full(len(live), FILL, dtype=np.uint8),
                  dig=np.full(20 * len(live), FILL, dtype=np.uint8))
        for k, v in up.items():
            self.bufs[k].upload(v)
        return live, fin

    def run_round(self, r):
        f, lib = self.feed, _capi.load()
        live, fin = self.upload_round(r)
        m = len(live)
        H.b64_update_launch(*self.args(m), stream=self.stream)
        _capi.check(lib.lbf_stream_synchronize(self.stream))
        osz = self.bufs["osz"].download(4 * m, dtype=np.uint32)
        ver = self.bufs["ver"].download(m)
        dig = self.bufs["dig"].download(20 * m).reshape(m, 20)
        for j, k in enumerate(live):
            c = f.chains[k]
            before = len(f.sofar[k])
            if fin[j]:
                f.model[k], f.sofar[k] = M.init(), c.want
                assert osz[j] == c.size and ver[j] == int(c.verdict), (c.desc, osz[j], c.size, ver[j])
                assert dig[j].tobytes() == sha1(c.want[:c.cap]), c.desc
            else:
                f.model[k], new = model_update(f.model[k], c.pieces[r])
                f.sofar[k] += new
                assert osz[j] == 0xEEEEEEEE and ver[j] == FILL and (dig[j] == FILL).all(), c.desc
            s, lo, hi = int(f.slot[k]), min(before, c.cap), min(len(f.sofar[k]), c.cap)
            f.want_out[s + lo:s + hi] = np.frombuffer(f.sofar[k][lo:hi], dtype=np.uint8)
        f.out = self.bufs["out"].download(f.out.size)
        wrong = np.flatnonzero(f.out != f.want_out)
        assert wrong.size == 0, f.where(int(wrong[0]))
        f.b64 = self.bufs["b64"].download(16 * len(f.chains)).view(B64_STATE_DTYPE)
        f.sha = self.bufs["sha"].download(96 * len(f.chains)).view(STATE_DTYPE)
        assert f.b64.tobytes() == M.b64_records(f.model, B64_STATE_DTYPE).tobytes()
        f.check_sha([r >= len(c.pieces) - 1 for c in f.chains])


def test_device_resident_launch_on_a_caller_stream():
    chains = _ragged_chains(65, 8065)
    feed = Feed(chains, sphase=0, tphase=4)
    text_max = max(feed.texts([k for k, c in enumerate(chains) if r < len(c.pieces)], r)[0].size
                   for r in range(feed.rounds))
    dev = DeviceFeed(feed, 65, text_max)
    try:
        dev.run_round(0)
        # an undersized array is refused, each in turn, before anything runs
        live, _ = dev.upload_round(1)
        m = len(live)
        assert m > 1
        elem = dict(so=4, toff=8, tlen=4, fin=1, ooff=8, caps=4, osz=4, dig=20, exp=20, ver=1, poff=8, psz=4)
        words = dict(so="state_of", toff="text_offsets", tlen="text_lens", fin="final", ooff="out_offsets", caps="caps",
                     osz="out_sizes", dig="digests", exp="expected", ver="verdicts", poff="piece_offsets",
                     psz="piece_sizes", b64="b64_states", sha="sha_states")
        small = {k: DeviceBuffer(e * (m - 1)) for k, e in elem.items()}
        small["b64"], small["sha"] = DeviceBuffer(16 * 64), DeviceBuffer(96 * 64)
        try:
            for k, b in small.items():
                with pytest.raises(LbfError) as e:
                    H.b64_update_launch(*dev.args(m, **{k: b}), stream=dev.stream)
                assert e.value.status == _capi.LBF_ERR_INVALID and words[k] in str(e.value), (k, str(e.value))
            with pytest.raises(LbfError) as e:
                H.b64_update_launch(*dev.args(m, b64=dev.bufs["b64"].ptr + 8), stream=dev.stream)
            assert "16-byte" in str(e.value)
        finally:
            for b in small.values():
                b.free()
        _capi.check(_capi.load().lbf_stream_synchronize(dev.stream))
        assert dev.bufs["out"].download(feed.out.size).tobytes() == feed.want_out.tobytes()
        for r in range(1, feed.rounds):
            dev.run_round(r)
        assert feed.b64.tobytes() == new_b64_states(65).tobytes() and feed.sha.tobytes() == new_states(65).tobytes()
    finally:
        dev.close()


def test_forged_device_records_write_nothing_outside_slot_and_records():
    """Records the launch cannot read, forged: ncarry = 255 and carry =
    0xFFFFFFFF count & 3 and masked; `decoded` anywhere up to 2^64 - 1, where
    decoded + 3g would wrap to a position before or inside the slot and the
    piece table's size to 4 GiB, is clamped to 2^61 and writes nothing.  The slot
    gets at most its cap bytes, the guard bytes around slots, records and tables
    stay, the piece table never names more than the slot holds, a piece that
    names no chain is skipped, and a chunk over 1 GiB decodes nothing and, on a
    final piece, leaves both records as new."""
    lib = _capi.load()
    n_states, cap = 9, 100
    n = n_states + 1
    big = (1 << 30) + 1
    t = W.xmlrpc_text(W.chunk_bytes(150, seed=6))  # decodes to more than the slot holds
    b64, sha = new_b64_states(n_states + 1), new_states(n_states + 1)  # one guard record behind each array
    b64["ncarry"], b64["carry"] = 255, 0xFFFFFFFF
    decoded = [0, 96, 99, 100, 3 << 40, 2**64 - 12, 2**64 - 1, 2**64 - 300, 0]
    b64["decoded"][:n_states] = np.array(decoded, dtype=np.uint64)
    b64.view(np.uint8).reshape(-1, 16)[n_states] = FILL
    sha.view(np.uint8).reshape(-1, 96)[n_states] = FILL
    slot = 64 + 256 * np.arange(n, dtype=np.uint64)
    out = np.full(64 + 256 * n, FILL, dtype=np.uint8)
    text = np.frombuffer(t + b"\0", dtype=np.uint8)
    state_of = np.arange(n, dtype=np.uint32)  # the last piece names no chain
    fin = np.array([0, 1, 0, 1, 0, 0, 1, 0, 1, 1], np.uint8)
    caps = np.full(n, cap, np.uint32)
    caps[8] = big
    host = dict(b64=b64, sha=sha, so=state_of, text=text, toff=np.zeros(n, np.uint64),
                tlen=np.full(n, len(t), np.uint32), fin=fin, out=out, ooff=slot, caps=caps,
                osz=np.full(n, 0xEEEEEEEE, np.uint32), dig=np.full(20 * n, FILL, np.uint8),
                exp=np.zeros(20 * n, np.uint8), ver=np.full(n, FILL, np.uint8),
                poff=np.full(n, 0xEEEEEEEE, np.uint64), psz=np.full(n, 0xEEEEEEEE, np.uint32))
    bufs = {k: DeviceBuffer(v.nbytes) for k, v in host.items()}
    try:
        for k, v in host.items():
            bufs[k].upload(v)
        H.b64_update_launch(bufs["b64"], bufs["sha"], n_states, bufs["so"], bufs["text"], bufs["toff"], bufs["tlen"],
                            bufs["fin"], n, bufs["out"], bufs["ooff"], bufs["caps"], bufs["osz"], bufs["dig"],
                            bufs["exp"], bufs["ver"], bufs["poff"], bufs["psz"])
        _capi.check(lib.lbf_device_synchronize())
        # the piece table the update kernel read: never more than what is left of the slot
        psz = bufs["psz"].download(4 * n, dtype=np.uint32)
        poff = bufs["poff"].download(8 * n, dtype=np.uint64)
        assert psz.tolist() == [100, 4, 1, 0, 0, 0, 0, 0, 0, 0xEEEEEEEE]
        assert poff[:8].tolist() == [int(slot[k]) + min(decoded[k], cap) for k in range(8)] and poff[8] == 0
        got = bufs["out"].download(out.size)
        for k in range(n):
            s = int(slot[k])
            assert (got[s - 64:s] == FILL).all() and (got[s + cap:s + 192] == FILL).all(), k
        assert (got[int(slot[1]):int(slot[1]) + 96] == FILL).all()   # chain 1 continues at byte 96
        for k in (3, 4, 5, 6, 7, 8, 9):  # at the cap, far past it, about to wrap, over 1 GiB, skipped: nothing written
            assert (got[int(slot[k]):int(slot[k]) + 192] == FILL).all(), k
        b2 = bufs["b64"].download(b64.nbytes).view(B64_STATE_DTYPE)
        s2 = bufs["sha"].download(sha.nbytes).view(STATE_DTYPE)
        assert b2[n_states].tobytes() == bytes([FILL]) * 16 and s2[n_states].tobytes() == bytes([FILL]) * 96
        assert (b2["ncarry"][:n_states] <= 3).all() and (b2["carry"][:n_states] < 1 << 18).all()
        assert b2[[1, 3, 6, 8]].tobytes() == new_b64_states(4).tobytes()  # the final pieces' records are as new,
        assert s2[[1, 3, 6, 8]].tobytes() == new_states(4).tobytes()      # both of each pair
        assert b2["decoded"][[5, 7]].tolist() == [1 << 61, 1 << 61]       # clamped: the host call refuses such a record
        assert s2["total"][[3, 4, 5, 7]].tolist() == [0, 0, 0, 0]         # and the hash absorbed nothing for them
        osz, ver = bufs["osz"].download(4 * n, dtype=np.uint32), bufs["ver"].download(n)
        E = 0xEEEEEEEE
        assert osz.tolist() == [E, cap + 1, E, cap + 1, E, E, cap + 1, E, 0, E]
        assert ver.tolist() == [FILL, 0, FILL, 0, FILL, FILL, 0, FILL, 0, FILL]
    finally:
        for b in bufs.values():
            b.free()


# ------------------------------------------------------------ 12. C++
def test_cpp_piece_hasher_update_text():
    out = subprocess.run([os.path.join(ROOT, "bitflood_amd", "lib", "lbf_piece_text_tests")], capture_output=True,
                         text=True, timeout=120)
    assert out.returncode == 0, out.stderr + out.stdout
    assert "piece_text_tests OK" in out.stdout

"""Chunks to send, base64-encoded and hashed piece by piece on the GPU: resumable
encoder states beside the resumable SHA-1 states (lbf_b64_enc_state,
lbf_b64_encode_update_launch / lbf_b64_encode_update_batch,
ChunkHasher.update_encode).

Expected values never come from a GPU path: whole texts from
tests/wire_layouts.xmlrpc_text (pinned to xmlrpc++'s recorded encoder output)
and base64.b64encode, what each piece writes and the records between pieces from
tests/wire_encode_model.py (pinned to those texts in tests/test_b64_encode_cpu.py),
digests from hashlib, SHA records from tests/sha1_model.py.  Every call is
checked whole: both record arrays, every byte of a 0xEE-filled text arena with
gaps between the slots -- the characters produced so far where they belong, 0xEE
everywhere else, a chain's characters that have not yet been produced included
-- new_offsets and new_lens, text sizes, digests and verdicts.
"""
import ast
import base64
import hashlib
import os
import subprocess
import sys

import numpy as np
import pytest

from bitflood_amd import B64_ENC_STATE_DTYPE, DeviceBuffer, LbfError, new_b64_enc_states, new_states
from bitflood_amd import hashing as H
from tests import large_index as L
from tests import sha1_model
from tests import wire_encode_model as E
from tests import wire_layouts as W

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL, MARK = 0xEE, 0xA5
T = E.TILE_BYTES  # the kernel's tile in bytes (tests/test_b64_encode_cpu.py reads it back from the source)
BOTH = (E.XMLRPC, E.FLAT)
MARK64, MARK32 = 0xA5A5A5A5A5A5A5A5, 0xA5A5A5A5


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


def whole(data: bytes, layout: int) -> bytes:
    return W.xmlrpc_text(data) if layout == E.XMLRPC else base64.b64encode(data)


def split(data: bytes, cuts):
    """data cut at the ascending positions `cuts`."""
    edges = [0] + list(cuts) + [len(data)]
    return [data[a:b] for a, b in zip(edges, edges[1:])]


def launch(enc, sha, state_of, data, offs, sizes, fin, text, toffs, caps, expected=None, n_states=None):
    """One lbf_b64_encode_update_launch over host arrays: records, data and tables
    up, the launch, everything back.  `enc`, `sha` and a numpy `text` are updated
    in place (a DeviceBuffer `text` stays on the device).  The outputs come back
    with MARK in every entry the launch did not write."""
    n = len(offs)
    arrays = {
        "enc": enc.view(np.uint8), "sha": sha.view(np.uint8),
        "so": None if state_of is None else np.ascontiguousarray(state_of, dtype=np.uint32),
        "data": np.concatenate([np.ascontiguousarray(data, dtype=np.uint8), np.zeros(16, dtype=np.uint8)]),
        "offs": np.ascontiguousarray(offs, dtype=np.uint64), "sizes": np.ascontiguousarray(sizes, dtype=np.uint32),
        "fin": None if fin is None else np.ascontiguousarray(fin).astype(bool).astype(np.uint8),
        "toffs": np.ascontiguousarray(toffs, dtype=np.uint64), "caps": np.ascontiguousarray(caps, dtype=np.uint32),
        "exp": None if expected is None else np.ascontiguousarray(expected, dtype=np.uint8).reshape(n, 20),
        "noff": np.full(n, MARK64, dtype=np.uint64), "nlen": np.full(n, MARK32, dtype=np.uint32),
        "tsize": np.full(n, MARK32, dtype=np.uint32), "dig": np.full((n, 20), MARK, dtype=np.uint8),
        "ver": np.full(n, MARK, dtype=np.uint8),
    }
    if not isinstance(text, DeviceBuffer):
        arrays["text"] = text
    dev = {}
    try:
        for name, a in arrays.items():
            if a is not None:
                dev[name] = DeviceBuffer(max(a.nbytes, 16))
                dev[name].upload(a)
        d_text = text if isinstance(text, DeviceBuffer) else dev["text"]
        H.b64_encode_update_launch(dev["enc"], dev["sha"], enc.size if n_states is None else n_states, dev.get("so"),
                                   dev["data"], dev["offs"], dev["sizes"], dev.get("fin"), n, d_text, dev["toffs"],
                                   dev["caps"], dev["noff"], dev["nlen"], dev["tsize"], dev["dig"], dev.get("exp"),
                                   dev["ver"] if expected is not None else None)
        H.synchronize()
        out = {}
        for name in ("noff", "nlen", "tsize", "dig", "ver", "enc", "sha") + (("text",) if "text" in arrays else ()):
            dev[name].download_into(arrays[name])
            out[name] = arrays[name]
        # the inputs are inputs
        for name in ("offs", "sizes", "toffs", "caps"):
            assert np.array_equal(dev[name].download(arrays[name].nbytes), arrays[name].view(np.uint8)), name
    finally:
        for b in dev.values():
            b.free()
    return out


class Chain:
    """One chunk as the pieces it is fed in, the last one final (or none, with
    final=False).  `cap` is the slot's size (default: the chunk's text length)."""

    def __init__(self, pieces, layout, cap=None, digest_ok=True, sphase=None, dphase=None, final=True, desc=""):
        self.pieces = [bytes(p) for p in pieces]
        self.data = b"".join(self.pieces)
        self.layout, self.final = layout, final
        self.text = whole(self.data, layout)
        self.cap = len(self.text) if cap is None else cap
        digest = sha1(self.data)
        self.expected = digest if digest_ok else bytes([digest[0] ^ 0x40]) + digest[1:]
        self.digest, self.digest_ok = digest, digest_ok
        self.sphase, self.dphase, self.desc = sphase, dphase, desc


class Feed:
    """Chains fed round by round (piece r of every chain that has one goes in
    call r) through the launch or through update_encode, everything checked after
    every call."""

    def __init__(self, chains, via, check_h=True, skipped=False):
        self.chains, self.via, self.check_h, self.skipped = chains, via, check_h, skipped
        n = len(chains)
        self.caps = np.array([c.cap for c in chains], dtype=np.uint32)
        self.slot = np.zeros(n, dtype=np.uint64)
        pos = 16
        for k, c in enumerate(chains):  # a gap in front of every slot; slots at the phase asked for
            pos += 1 + k % 3
            if c.sphase is not None:
                pos += (c.sphase - pos) % 16
            self.slot[k] = pos
            pos += c.cap
        self.text = np.full(pos + 48, FILL, dtype=np.uint8)
        self.want_text = self.text.copy()
        self.enc, self.sha = new_b64_enc_states(n), new_states(n)
        for k, c in enumerate(chains):
            self.enc["layout"][k] = c.layout
        self.model = [E.init(c.layout) for c in chains]
        self.sha_model = [sha1_model.init() for _ in chains]
        self.fed = [b""] * n
        self.expected = np.frombuffer(b"".join(c.expected for c in chains), dtype=np.uint8).reshape(n, 20)
        self.rounds = max(len(c.pieces) for c in chains)

    def run(self, hasher=None):
        for r in range(self.rounds):
            self.run_round(r, hasher)
        for k, c in enumerate(self.chains):  # every slot holds the whole chunk's text, as far as it fits
            if c.final:
                s = int(self.slot[k])
                m = min(c.cap, len(c.text))
                assert self.text[s:s + m].tobytes() == c.text[:m], c.desc

    def run_round(self, r, hasher=None):
        live = [k for k, c in enumerate(self.chains) if r < len(c.pieces)]
        fin = [self.chains[k].final and r == len(self.chains[k].pieces) - 1 for k in live]
        parts, offs, pos = [], [], 0
        for k in live:
            c = self.chains[k]
            pad = 1 if c.dphase is None else (c.dphase - pos) % 16
            parts.append(bytes([0x5A] * pad) + c.pieces[r])
            offs.append(pos + pad)
            pos += pad + len(c.pieces[r])
        data = np.frombuffer(b"".join(parts) + b"\x5A", dtype=np.uint8)
        sizes = [len(self.chains[k].pieces[r]) for k in live]
        m = len(live)
        if self.via == "batch":
            noff, nlen, tsize, ver = hasher.update_encode(self.enc, self.sha, data, offs, sizes, self.text,
                                                          self.slot[live], self.caps[live], state_of=live, final=fin,
                                                          expected=self.expected[live])
            dig, untouched = None, (0, False)
        else:
            so, toffs, caps, exp = list(live), list(self.slot[live]), list(self.caps[live]), self.expected[live]
            if self.skipped:  # one more piece that names no chain: were it taken, it would write at the arena's start
                so, offs, sizes, fin = so + [len(self.chains)], offs + [0], sizes + [5], fin + [True]
                toffs, caps, exp = toffs + [0], caps + [100], np.concatenate([exp, exp[:1]])
            out = launch(self.enc, self.sha, so, data, offs, sizes, fin, self.text, toffs, caps, exp)
            noff, nlen, tsize, dig, ver = out["noff"], out["nlen"], out["tsize"], out["dig"], out["ver"]
            untouched = (MARK32, MARK)
            if self.skipped:
                assert noff[m] == MARK64 and nlen[m] == MARK32 and tsize[m] == MARK32 and ver[m] == MARK
                assert (dig[m] == MARK).all()
        bad = []
        for j, k in enumerate(live):
            c = self.chains[k]
            piece = c.pieces[r]
            self.model[k], at, chars, length = E.update(self.model[k], piece, fin[j])
            lo, clipped = E.clip(at, chars, c.cap)
            s = int(self.slot[k])
            self.want_text[s + lo:s + lo + len(clipped)] = np.frombuffer(clipped, dtype=np.uint8)
            if int(noff[j]) != s + lo or int(nlen[j]) != len(clipped):
                bad.append((k, c.desc, "new", int(noff[j]), s + lo, int(nlen[j]), len(clipped)))
            if fin[j]:
                fits = length <= c.cap
                want = (length if fits else c.cap + 1, fits and c.digest_ok)
                if (int(tsize[j]), bool(ver[j])) != want or ver[j] not in (0, 1):
                    bad.append((k, c.desc, "final", int(tsize[j]), int(ver[j]), want))
                if dig is not None and dig[j].tobytes() != c.digest:
                    bad.append((k, c.desc, "digest"))
                self.sha_model[k], self.fed[k] = sha1_model.init(), b""
            else:
                if (tsize[j], ver[j]) != untouched or (dig is not None and not (dig[j] == MARK).all()):
                    bad.append((k, c.desc, "not final", int(tsize[j]), int(ver[j])))
                self.fed[k] += piece
                if self.check_h:
                    self.sha_model[k] = sha1_model.update(self.sha_model[k], piece)
        assert not bad, bad[:5]
        wrong = np.flatnonzero(self.text != self.want_text)
        assert wrong.size == 0, (wrong[:8].tolist(), self.where(int(wrong[0])))
        want_enc = np.array([E.record(st) for st in self.model], dtype=B64_ENC_STATE_DTYPE)
        assert self.enc.tobytes() == want_enc.tobytes(), next(
            (self.chains[k].desc, self.enc[k], want_enc[k]) for k in range(len(self.chains))
            if self.enc[k].tobytes() != want_enc[k].tobytes())
        fresh = new_states(1)[0]
        for k, c in enumerate(self.chains):
            st, fed = self.sha[k], self.fed[k]
            if not fed:
                assert st.tobytes() == fresh.tobytes() or (st["total"] == 0 and st["buffered"] == 0
                                                           and st["h"].tobytes() == fresh["h"].tobytes()), c.desc
                continue
            b = len(fed) % 64
            assert st["total"] == len(fed) and st["buffered"] == b, (c.desc, st)
            assert st["block"][:b].tobytes() == fed[len(fed) - b:], c.desc
            if self.check_h:
                assert list(st["h"]) == list(self.sha_model[k][0]), c.desc

    def where(self, at):
        for k, c in enumerate(self.chains):
            s = int(self.slot[k])
            if s <= at < s + c.cap:
                return f"chain {k} ({c.desc}) text position {at - s} of {len(c.text)}, slot phase {s % 16}"
        return f"arena byte {at}, outside every slot"


def feed(chains, via, hasher, **kw):
    Feed(chains, via, **kw).run(hasher)


VIAS = ("launch", "batch")


# ------------------------------------------------------------ 1. every cut
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_every_cut_of_167_bytes(hasher, layout, via):
    """168 chains x 2 pieces in one pair of calls: three lines and a 5-byte tail."""
    d = W.chunk_bytes(167)
    feed([Chain(split(d, [a]), layout, desc=f"cut at {a}") for a in range(168)], via, hasher)


# ------------------------------------------------------------ 2. one period of lines against blocks
@pytest.mark.parametrize("layout", BOTH)
def test_pieces_start_at_every_byte_of_a_period(hasher, layout):
    """864 bytes are 16 lines, 1,168 characters: the lcm of the 73-character line
    and the 16-byte block.  Chain a's second piece starts at byte a and its third
    at byte a + 900, slots at all 16 text phases and data at all 16 source phases
    for each: every (ncarry, column, block phase) triple, twice."""
    d = W.chunk_bytes(1800 + 2, seed=layout)
    chains = [Chain(split(d, [a, a + 900]), layout, sphase=a % 16, dphase=(a // 16) % 16, desc=f"period a={a}")
              for a in range(864)]
    assert {(c.sphase, c.dphase) for c in chains} == {(x, y) for x in range(16) for y in range(16)}
    feed(chains, "launch", hasher, check_h=False)


# ------------------------------------------------------------ 3. tile edges
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_cuts_around_tile_edges(hasher, layout, via):
    d = W.chunk_bytes(3 * T + 100, seed=3)
    chains, n = [], 0
    for k in (1, 2, 3):
        for dd in range(-3, 4):
            chains.append(Chain(split(d, [k * T + dd]), layout, sphase=(0, 1, 8, 15)[n % 4], dphase=(5 * n) % 16,
                                desc=f"cut at {k}T{dd:+d}"))
            n += 1
    for dd in range(-3, 4):  # the same cuts taken as three pieces
        chains.append(Chain(split(d, [T + dd, 2 * T + dd]), layout, sphase=n % 16, dphase=0, desc=f"1T,2T{dd:+d}"))
        chains.append(Chain(split(d, [2 * T + dd, 3 * T + dd]), layout, sphase=0, dphase=n % 16, desc=f"2T,3T{dd:+d}"))
        n += 1
    feed(chains, via, hasher)


# ------------------------------------------------------------ 4. degenerate pieces
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_degenerate_pieces(hasher, layout, via):
    d = W.chunk_bytes(64, seed=4)
    shapes = [[1, 1, 1], [1, 1, 1, 1, 1, 1, 1], [0, 1, 2, 3], [3, 2, 1, 0], [2, 0, 1], [0, 0, 0], [0], [3, 0], [4, 0],
              [5, 0], [1, 0, 0], [2, 2, 2, 0], [53, 1, 0], [52, 1, 1, 1], [54], [54, 0], [1], [2], [3]]
    chains = []
    for s in shapes:
        edges = np.cumsum(s)
        chains.append(Chain(split(d[:int(edges[-1])], edges[:-1].tolist()), layout, desc=f"pieces {s}"))
    chains.append(Chain(split(d, [1, 2, 3]), layout, final=False, desc="never final"))
    assert any(len(c.data) == 0 for c in chains)  # a 0-byte chunk
    feed(chains, via, hasher)


# ------------------------------------------------------------ 5. both layouts and a skipped piece in one launch
def test_mixed_layouts_and_a_skipped_piece(hasher):
    d = W.chunk_bytes(2 * T + 77, seed=5)
    chains = [Chain(split(d[:n], [n // 3, n // 2]), layout, sphase=(3 * n) % 16, desc=f"{n} B layout {layout}")
              for n in (0, 5, 167, 864, T, T + 1, 2 * T + 77) for layout in BOTH]
    feed(chains, "launch", hasher, skipped=True)


# ------------------------------------------------------------ 6. caps
@pytest.mark.parametrize("via", VIAS)
@pytest.mark.parametrize("layout", BOTH)
def test_caps(hasher, layout, via):
    """The cap is the text length, one less, and 0 (and a few more): nothing at or
    past it is written, text_sizes == cap + 1, verdict 0, new_lens clipped."""
    chains = []
    for size, cuts in ((167, [50, 110]), (T + 200, [T - 1, T + 100]), (54, [53]), (2, [1])):
        d = W.chunk_bytes(size, seed=6)
        full = E.text_length(size, layout)
        for cap in sorted({full, full - 1, 0, full // 2, max(full - 16, 0), full - 4, full + 7}):
            chains.append(Chain(split(d, cuts), layout, cap=cap, sphase=cap % 16, desc=f"{size} B cap {cap} of {full}"))
    assert any(c.cap == len(c.text) - 1 for c in chains) and any(c.cap == 0 for c in chains)
    feed(chains, via, hasher)


def test_cap_over_the_bound_is_refused_on_the_device():
    """A cap above lbf_b64_text_length(1 GiB, xmlrpc): nothing encoded, the hash
    gets an empty piece; a final piece gets verdict 0 and text size 0 and both
    records restart, a piece that is not final leaves them as they were."""
    d = np.frombuffer(W.chunk_bytes(300, seed=7), dtype=np.uint8)
    for layout in BOTH:
        enc, sha = new_b64_enc_states(3, layout), new_states(3)
        text = np.full(1024, FILL, dtype=np.uint8)
        # bring chains 0 and 1 to 100 bytes, honestly
        launch(enc, sha, None, d, [0, 0, 0], [100, 100, 100], [0, 0, 0], text, [16, 336, 656], [300, 300, 300],
               np.zeros((3, 20), dtype=np.uint8))
        before_enc, before_sha, before_text = enc.copy(), sha.copy(), text.copy()
        assert (enc["taken"] == 100).all()
        big = E.MAX_TEXT_CAP + 1
        exp = np.frombuffer(sha1(d[:100]) * 3, dtype=np.uint8).reshape(3, 20)  # the digest an empty last piece leaves
        out = launch(enc, sha, None, d, [100, 100, 100], [50, 50, 50], [1, 0, 1], text, [16, 336, 656],
                     [big, big, 300], exp)
        assert np.array_equal(text[:656], before_text[:656])  # the refused slots: untouched
        assert out["nlen"].tolist()[:2] == [0, 0] and out["noff"].tolist()[:2] == [16, 336]
        assert out["tsize"][0] == 0 and out["ver"][0] == 0 and out["tsize"][1] == MARK32 and out["ver"][1] == MARK
        assert out["dig"][0].tobytes() == sha1(d[:100])  # the hash took an empty piece
        fresh_enc, fresh_sha = new_b64_enc_states(1, layout), new_states(1)
        assert enc[0].tobytes() == fresh_enc[0].tobytes() and sha[0].tobytes() == fresh_sha[0].tobytes()
        assert enc[1].tobytes() == before_enc[1].tobytes() and sha[1].tobytes() == before_sha[1].tobytes()
        # the honest neighbour ends its chunk of 150 bytes; its digest is no digest of 100 bytes
        want = whole(d[:150].tobytes(), layout)
        assert text[656:656 + len(want)].tobytes() == want and (text[656 + len(want):] == FILL).all()
        assert out["tsize"][2] == len(want) and out["ver"][2] == 0 and out["dig"][2].tobytes() == sha1(d[:150])


# ------------------------------------------------------------ 7. forged records
def test_forged_records_stay_inside_their_slot_and_records():
    d = np.frombuffer(W.chunk_bytes(400, seed=8), dtype=np.uint8)
    forged = [dict(taken=1 << 63, carry=0xFFFFFFFF, ncarry=3, layout=7, zero=0xFFFF),
              dict(taken=100, carry=0xFFFFFFFF, ncarry=3, layout=7, zero=1),     # really ncarry 1, layout 1
              dict(taken=56, carry=0xDEADBEEF, ncarry=0, layout=2, zero=0),      # really ncarry 2, layout 0
              dict(taken=(1 << 61) - 1, carry=0x1234, ncarry=1, layout=0, zero=0),
              dict(taken=0xFFFFFFFFFFFFFFFF, carry=7, ncarry=255, layout=255, zero=9)]
    n = len(forged)
    for fin in (0, 1):
        enc, sha = new_b64_enc_states(n + 1), new_states(n + 1)
        for k, f in enumerate(forged):
            for name, v in f.items():
                enc[name][k] = v
        cap, slots = 400, [16 + 450 * k for k in range(n + 1)]
        text = np.full(16 + 450 * (n + 1), FILL, dtype=np.uint8)
        want_text = text.copy()
        guard_enc, guard_sha = enc[n].copy(), sha[n].copy()
        sizes = [200, 100, 7, 50, 9]
        out = launch(enc, sha, list(range(n)), d, [3 * k for k in range(n)], sizes, [fin] * n, text, slots[:n],
                     [cap] * n, np.zeros((n, 20), dtype=np.uint8))
        for k, f in enumerate(forged):
            state = E.sanitize(f["taken"], f["carry"], f["ncarry"], f["layout"])
            after, at, chars, length = E.update(state, d[3 * k:3 * k + sizes[k]].tobytes(), bool(fin))
            lo, clipped = E.clip(at, chars, cap)
            want_text[slots[k] + lo:slots[k] + lo + len(clipped)] = np.frombuffer(clipped, dtype=np.uint8)
            assert (int(out["noff"][k]), int(out["nlen"][k])) == (slots[k] + lo, len(clipped)), k
            assert tuple(enc[k]) == E.record(after), (k, enc[k])
            if fin:
                assert out["tsize"][k] == (length if length <= cap else cap + 1) and out["ver"][k] == 0, k
            else:
                assert out["tsize"][k] == MARK32 and out["ver"][k] == MARK, k
        assert np.array_equal(text, want_text), np.flatnonzero(text != want_text)[:8]
        assert enc[n].tobytes() == guard_enc.tobytes() and sha[n].tobytes() == guard_sha.tobytes()  # the neighbour's
    assert any(len(E.clip(*E.update(E.sanitize(**{k: v for k, v in f.items() if k != "zero"}), b"x" * 50)[1:3],
                          400)[1]) for f in forged)  # some of them do write


# ------------------------------------------------------------ 8. one wrong digest in a batch
@pytest.mark.parametrize("via", VIAS)
def test_one_wrong_expected_digest(hasher, via):
    d = W.chunk_bytes(1000, seed=9)
    chains = [Chain(split(d[:200 + 100 * k], [77]), k % 2, digest_ok=k != 3, desc=f"chain {k}") for k in range(7)]
    f = Feed(chains, via)
    f.run(hasher)  # only chain 3's verdict is 0 (checked per call); its text is complete all the same
    s = int(f.slot[3])
    assert f.text[s:s + chains[3].cap].tobytes() == chains[3].text


# ------------------------------------------------------------ 9. the batch call
def test_batch_refusals_leave_everything_untouched(hasher):
    d = np.frombuffer(W.chunk_bytes(600, seed=10), dtype=np.uint8)

    def fresh():
        enc, sha = new_b64_enc_states(3), new_states(3)
        text = np.full(1000, FILL, dtype=np.uint8)
        hasher.update_encode(enc, sha, d, [0, 0, 0], [100, 100, 100], text, [0, 300, 600], [300, 300, 300])
        return enc, sha, text

    ok = dict(offsets=[100, 100, 100], sizes=[50, 50, 50], text_offsets=[0, 300, 600], text_caps=[300, 300, 300],
              state_of=[0, 1, 2], final=[1, 0, 1])
    cases = [
        (dict(offsets=[100, 551, 100]), None, "piece 1 lies outside"),
        (dict(text_offsets=[0, 300, 701]), None, "piece 2 has its slot outside"),
        (dict(state_of=[0, 3, 2]), None, "piece 1 names state 3"),
        (dict(state_of=[0, 1, 0]), None, "piece 2 is the second piece of state 0"),
        (dict(text_offsets=[0, 299, 600]), None, "piece 1 has a slot that overlaps"),
        (dict(text_caps=[300, E.MAX_TEXT_CAP + 1, 300]), None, "piece 1 has a text slot"),
        ({}, ("enc", 1, "ncarry", 2), "piece 1 continues a corrupt state: ncarry 2"),
        ({}, ("enc", 1, "carry", 0x100), "carry holds more"),
        ({}, ("enc", 2, "layout", 2), "piece 2 continues a corrupt state: layout 2"),
        ({}, ("enc", 0, "zero", 1), "zero field"),
        ({}, ("enc", 0, "taken", 103), "SHA state total 100 is not taken 103"),
        ({}, ("sha", 2, "buffered", 37), "SHA state is corrupt"),
        ({}, ("enc+sha", 1, "taken", (1 << 30) - 49), "more than 1 GiB"),
    ]
    for change, spoil, message in cases:
        enc, sha, text = fresh()
        if spoil:
            which, k, name, v = spoil
            if which == "enc+sha":  # a consistent pair at the edge of the bound
                enc["taken"][k], enc["ncarry"][k], enc["carry"][k] = v, v % 3, 0
                sha["total"][k], sha["buffered"][k] = v, v % 64
            else:
                (enc if which == "enc" else sha)[name][k] = v
        before = enc.copy(), sha.copy(), text.copy()
        args = {**ok, **change}
        with pytest.raises(LbfError) as e:
            hasher.update_encode(enc, sha, d, args["offsets"], args["sizes"], text, args["text_offsets"],
                                 args["text_caps"], state_of=args["state_of"], final=args["final"],
                                 expected=np.zeros((3, 20), dtype=np.uint8))
        assert e.value.status == -1 and message in str(e.value), (message, str(e.value))
        assert enc.tobytes() == before[0].tobytes() and sha.tobytes() == before[1].tobytes()
        assert np.array_equal(text, before[2])
    enc, sha, text = fresh()  # and the accepted call goes through
    hasher.update_encode(enc, sha, d, text=text, **{k: v for k, v in ok.items() if k != "final"})
    assert (enc["taken"] == 150).all()


def split_run(h):
    """A 100-byte chunk and one of 3 MiB + 7 bytes, each in one final piece, both
    layouts: [(sha1 of the text arena, new_offsets, new_lens, text_sizes, verdicts, records)]."""
    d = np.random.default_rng(12).integers(0, 256, (3 << 20) + 7 + 100, dtype=np.uint8)
    exp = np.frombuffer(sha1(d[:100]) + sha1(d[100:]), dtype=np.uint8)
    out = []
    for layout in ("xmlrpc", "flat"):
        enc, sha = new_b64_enc_states(2, layout), new_states(2)
        text = np.full(5 << 20, FILL, dtype=np.uint8)
        r = h.update_encode(enc, sha, d, [0, 100], [100, (3 << 20) + 7], text, [5, 1000], [200, 4400000],
                            final=[1, 1], expected=exp)
        out.append((hashlib.sha1(text.tobytes()).hexdigest(), r[0].tolist(), r[1].tolist(), r[2].tolist(),
                    r[3].tolist(), enc.tobytes().hex() + sha.tobytes().hex()))
    return out


_SPLIT_CHILD = """
import sys
sys.path.insert(0, sys.argv[1])
from bitflood_amd import ChunkHasher
from tests.test_gpu_b64_encode import split_run
with ChunkHasher() as h:
    print(repr(split_run(h)))
"""


def test_update_mb_splits_a_large_piece_to_the_same_text(hasher):
    """LBF_UPDATE_MB=1 (read at context creation: a fresh child process) cuts a
    3 MiB piece over four launches; text, new_offsets / new_lens, sizes, verdicts
    and records are those of the unsplit call, and the text is the reference's."""
    r = subprocess.run([sys.executable, "-c", _SPLIT_CHILD, ROOT], capture_output=True, text=True, timeout=120,
                       env={**os.environ, "LBF_UPDATE_MB": "1"}, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    cut = ast.literal_eval(r.stdout.strip().splitlines()[-1])  # the child's repr of plain lists
    assert cut == split_run(hasher)
    d = np.random.default_rng(12).integers(0, 256, (3 << 20) + 7 + 100, dtype=np.uint8).tobytes()
    for layout, got in zip(BOTH, cut):
        text = np.full(5 << 20, FILL, dtype=np.uint8)
        a, b = whole(d[:100], layout), whole(d[100:], layout)
        text[5:5 + len(a)] = np.frombuffer(a, dtype=np.uint8)
        text[1000:1000 + len(b)] = np.frombuffer(b, dtype=np.uint8)
        assert got[0] == hashlib.sha1(text.tobytes()).hexdigest()
        assert got[1:5] == ([5, 1000], [len(a), len(b)], [len(a), len(b)], [True, True])
        assert got[5] == new_b64_enc_states(2, layout).tobytes().hex() + new_states(2).tobytes().hex()


# ------------------------------------------------------------ 10. 64-bit addresses
def test_text_slot_across_byte_2_to_the_32():
    """A text arena of 4 GiB + 1 MiB, the middle chain's slot straddling byte
    2^32: with a text address kept in 32 bits the characters past the line would
    land in the arena's first bytes (which stay 0xEE) and the slot would miss
    them -- wrong text, no fault."""
    d = W.chunk_bytes(T + 500, seed=13)
    buf = DeviceBuffer(L.LINE + (1 << 20))
    for layout in BOTH:
        chains = [Chain(split(d[:300], [100]), layout), Chain(split(d, [T // 2 + 1]), layout),
                  Chain(split(d[:700], [333]), layout)]
        caps = [c.cap for c in chains]
        slots = L.slot_case(caps, 1, L.STRADDLE, FILL)
        assert slots.kinds() == [L.BELOW, L.STRADDLE, L.ABOVE]
        try:
            for offset, data in slots.uploads():
                buf.upload(data, offset)
            enc, sha = new_b64_enc_states(3, layout), new_states(3)
            want_window = slots.window.copy()
            for r in (0, 1):
                pieces = [c.pieces[r] for c in chains]
                offs = np.cumsum([0] + [len(p) + 1 for p in pieces])[:3]
                data = np.frombuffer(b"\x5A".join(pieces), dtype=np.uint8)
                exp = np.frombuffer(b"".join(c.expected for c in chains), dtype=np.uint8).reshape(3, 20)
                out = launch(enc, sha, None, data, offs, [len(p) for p in pieces], [r] * 3, buf, slots.offsets, caps,
                             exp)
                for k, c in enumerate(chains):
                    at = E.pos(len(c.pieces[0]) // 3, layout) if r else 0
                    end = len(c.text) if r else E.pos(len(c.pieces[0]) // 3, layout)
                    assert (int(out["noff"][k]), int(out["nlen"][k])) == (int(slots.offsets[k]) + at, end - at), k
                    a = int(slots.offsets[k]) - slots.lo
                    want_window[a + at:a + end] = np.frombuffer(c.text[at:end], dtype=np.uint8)
                    if r:
                        assert out["tsize"][k] == len(c.text) and out["ver"][k] == 1, k
                assert np.array_equal(buf.download(slots.window.size, slots.lo), want_window), (layout, r)
                assert (buf.download(slots.alias.size, 0) == FILL).all(), (layout, r)
        except BaseException:
            buf.free()
            raise
    buf.free()

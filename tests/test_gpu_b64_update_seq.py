"""Several pieces of one chain's base64 text decoded and absorbed in one call,
in order, on the GPU: lbf_b64_update_seq_launch (one workgroup per chain, the
decoder's record in registers from the chain's first piece to its last; three
enqueues whatever the piece count) and lbf_b64_update_seq_batch /
ChunkHasher.update_text_seq.

Two yardsticks, both bit-exact.  Expected bytes, lengths, work arrays and
records come from tests/wire_piece_model.py, tests/wire_layouts.py,
tests/sha1_model.py and hashlib -- never from a GPU path; and everything the
new launch gives (both records, out_sizes, digests, verdicts, the work arrays,
every byte of the output arena) is held against what the same pieces give when
fed one per launch through lbf_b64_update_launch.  The arenas are pre-filled
with 0xEE, so nothing written outside the decoded range, or at or past the
cap, goes unnoticed.
"""
import base64
import hashlib

import numpy as np
import pytest

from bitflood_amd import (B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, LbfError, _capi, new_b64_states, new_states)
from bitflood_amd import hashing as H
from tests import sha1_model
from tests import wire_layouts as W
from tests import wire_piece_model as M

pytestmark = pytest.mark.gpu

FILL = 0xEE
TILE = 3888  # bytes of a decode tile (b64_update_stages.hpp)
BIG = (1 << 30) + 1  # a chunk size the decode refuses
SWITCHES = [(1, 0), (1, 1), (0, 1), (0, 0)]  # (lines, flat)


def sha1(b) -> bytes:
    return hashlib.sha1(bytes(b)).digest()


@pytest.fixture
def switches():
    """Sets the line/flat switches for a test and puts them back."""
    before = []

    def set_to(lines, flat):
        if not before:
            before.extend([H.set_b64_lines(lines), H.set_b64_flat(flat)])
        else:
            H.set_b64_lines(lines)
            H.set_b64_flat(flat)
    yield set_to
    if before:
        H.set_b64_lines(before[0])
        H.set_b64_flat(before[1])


def text_of(data: bytes, layout: str) -> bytes:
    """A chunk's text as xmlrpc++ peers send it (lines) or as the Java and Perl peers do (unbroken)."""
    return W.xmlrpc_text(data) if layout == "xmlrpc" else base64.b64encode(data)


def cut(text: bytes, at) -> list:
    at = [0] + sorted(min(max(int(a), 0), len(text)) for a in at) + [len(text)]
    return [text[a:b] for a, b in zip(at[:-1], at[1:])]


class Chain:
    """One state pair's pieces in a call.  `finals[j]` ends a chunk at piece j;
    `caps[j]` is the chunk size piece j names (one value for the chain, but for
    a refused piece); `digest_ok` false gives the final pieces a wrong expected digest."""

    def __init__(self, state, pieces, finals=None, cap=None, caps=None, digest_ok=True, desc=""):
        self.state, self.pieces, self.desc, self.digest_ok = state, [bytes(p) for p in pieces], desc, digest_ok
        self.finals = [False] * (len(pieces) - 1) + [True] if finals is None else list(finals)
        if cap is None:
            cap = len(W.decode(b"".join(self.pieces)))
        self.cap = cap
        self.caps = [cap] * len(pieces) if caps is None else list(caps)


class Scene:
    """Chains laid out for the device: pieces in table order (chain after
    chain), a chain's text in one run starting at its own phase mod 16, slots
    with guard bytes between them, and everything the models expect.  Every
    chunk of a chain (a final in mid-run starts the next) has a slot of its
    own: the hash runs behind the decode of the whole launch, so a chunk's
    bytes must still lie in its slot then."""

    def __init__(self, chains, n_states):
        self.chains, self.n_states = chains, n_states
        text, pos = [], 0
        self.toff, self.tlen, self.fin, self.slot, self.cap, self.first = [], [], [], [], [], [0]
        opos = 32
        for k, c in enumerate(chains):
            pad = (k * 7 - pos) % 16
            text.append(bytes(pad))
            pos += pad
            c.slots, new_chunk = [], True
            for p, f, cp in zip(c.pieces, c.finals, c.caps):
                if new_chunk:
                    opos = (opos + 15) // 16 * 16 + (5 * k) % 16
                    c.slots.append(opos)
                    opos += c.cap + 9
                new_chunk = bool(f)
                self.toff.append(pos)
                self.tlen.append(len(p))
                self.fin.append(1 if f else 0)
                self.slot.append(c.slots[-1])
                self.cap.append(cp)
                text.append(p)
                pos += len(p)
            c.slot = c.slots[0] if c.slots else opos
            self.first.append(len(self.toff))
        self.n = len(self.toff)
        self.text = np.frombuffer(b"".join(text) + bytes(16), dtype=np.uint8).copy()
        self.out_len = opos + 32
        self.model()

    def model(self):
        n = self.n
        self.want_out = np.full(self.out_len, FILL, dtype=np.uint8)
        self.want_osize = np.full(n, FILL * 0x01010101, dtype=np.uint32)
        self.want_poff = np.zeros(n, dtype=np.uint64)
        self.want_psize = np.zeros(n, dtype=np.uint32)
        self.want_dig = [None] * n
        self.want_ver = [None] * n
        self.expected = np.zeros((n, 20), dtype=np.uint8)
        self.want_b64, self.want_sha = {}, {}
        i = 0
        for c in self.chains:
            st, sofar, absorbed = M.init(), b"", b""
            for p, f, cp in zip(c.pieces, c.finals, c.caps):
                slot = self.slot[i]
                if cp > (1 << 30):  # refused: nothing decoded, an empty piece for the hash, verdict 0
                    size = 0
                else:
                    before = len(sofar)
                    st, new = M.update(st, p)
                    sofar += new
                    lo, hi = min(before, cp), min(len(sofar), cp)
                    self.want_out[slot + lo:slot + hi] = np.frombuffer(sofar[lo:hi], dtype=np.uint8)
                    absorbed += sofar[lo:hi]
                    self.want_poff[i], self.want_psize[i] = slot + lo, hi - lo
                    size = len(sofar) if len(sofar) <= cp else cp + 1
                if f:
                    d = sha1(absorbed)
                    self.want_dig[i] = d
                    self.want_osize[i] = size
                    exp = d if c.digest_ok else bytes([d[0] ^ 0x40]) + d[1:]
                    self.expected[i] = np.frombuffer(exp, dtype=np.uint8)
                    self.want_ver[i] = 1 if (c.digest_ok and cp <= (1 << 30) and size == cp) else 0
                    st, sofar, absorbed = M.init(), b"", b""
                i += 1
            self.want_b64[c.state] = st
            self.want_sha[c.state] = sha1_model.update(sha1_model.init(), absorbed)

    def upload(self):
        arrays = dict(b64=new_b64_states(self.n_states), sha=new_states(self.n_states), text=self.text,
                      toff=np.array(self.toff, dtype=np.uint64), tlen=np.array(self.tlen, dtype=np.uint32),
                      fin=np.array(self.fin, dtype=np.uint8), out=np.full(self.out_len, FILL, dtype=np.uint8),
                      slot=np.array(self.slot, dtype=np.uint64), cap=np.array(self.cap, dtype=np.uint32),
                      osize=np.full(self.n, FILL, dtype=np.uint8).repeat(4), dig=np.full(20 * self.n, FILL, np.uint8),
                      exp=self.expected, ver=np.full(self.n, FILL, dtype=np.uint8),
                      poff=np.full(8 * self.n, FILL, dtype=np.uint8), psize=np.full(4 * self.n, FILL, dtype=np.uint8),
                      cs=np.array([c.state for c in self.chains], dtype=np.uint32),
                      cf=np.array(self.first, dtype=np.uint32))
        bufs = {}
        for k, a in arrays.items():
            bufs[k] = DeviceBuffer(max(a.nbytes, 16))
            if a.nbytes:
                bufs[k].upload(a)
        return bufs

    @staticmethod
    def download(bufs, n, n_states, out_len):
        return dict(b64=bufs["b64"].download(16 * n_states).view(B64_STATE_DTYPE),
                    sha=bufs["sha"].download(96 * n_states).view(STATE_DTYPE), out=bufs["out"].download(out_len),
                    osize=bufs["osize"].download(4 * n).view(np.uint32), dig=bufs["dig"].download(20 * n).reshape(n, 20),
                    ver=bufs["ver"].download(n), poff=bufs["poff"].download(8 * n).view(np.uint64),
                    psize=bufs["psize"].download(4 * n).view(np.uint32))

    def run_seq(self):
        """ONE lbf_b64_update_seq_launch over the whole table."""
        bufs = self.upload()
        try:
            H.b64_update_seq_launch(bufs["b64"], bufs["sha"], self.n_states, bufs["cs"], bufs["cf"], len(self.chains),
                                    bufs["text"], bufs["toff"], bufs["tlen"], bufs["fin"], self.n, bufs["out"],
                                    bufs["slot"], bufs["cap"], bufs["osize"], bufs["dig"], bufs["exp"], bufs["ver"],
                                    bufs["poff"], bufs["psize"])
            H.synchronize()
            return self.download(bufs, self.n, self.n_states, self.out_len)
        finally:
            for b in bufs.values():
                b.free()

    def run_one_per_launch(self):
        """The existing route, one piece per launch of lbf_b64_update_launch:
        piece r of every chain that has one, round by round, each launch over
        the same arrays at the piece's table position and naming the chain's
        state."""
        bufs = self.upload()
        try:
            rounds = max(len(c.pieces) for c in self.chains)
            for r in range(rounds):
                for k in [k for k, c in enumerate(self.chains) if r < len(c.pieces)]:
                    i = self.first[k] + r
                    H.b64_update_launch(bufs["b64"], bufs["sha"], self.n_states, bufs["cs"].ptr + 4 * k, bufs["text"],
                                        bufs["toff"].ptr + 8 * i, bufs["tlen"].ptr + 4 * i, bufs["fin"].ptr + i, 1,
                                        bufs["out"], bufs["slot"].ptr + 8 * i, bufs["cap"].ptr + 4 * i,
                                        bufs["osize"].ptr + 4 * i, bufs["dig"].ptr + 20 * i, bufs["exp"].ptr + 20 * i,
                                        bufs["ver"].ptr + i, bufs["poff"].ptr + 8 * i, bufs["psize"].ptr + 4 * i)
            H.synchronize()
            return self.download(bufs, self.n, self.n_states, self.out_len)
        finally:
            for b in bufs.values():
                b.free()

    def check_against_models(self, got):
        wrong = np.flatnonzero(got["out"] != self.want_out)
        assert wrong.size == 0, (wrong[:8].tolist(), self.where(int(wrong[0])))
        bad = []
        i = 0
        for c in self.chains:
            for j, (f, cp) in enumerate(zip(c.finals, c.caps)):
                if cp > (1 << 30):
                    ok = got["poff"][i] == 0 and got["psize"][i] == 0
                else:
                    ok = got["poff"][i] == self.want_poff[i] and got["psize"][i] == self.want_psize[i]
                if f:
                    ok = ok and got["osize"][i] == self.want_osize[i] and got["dig"][i].tobytes() == self.want_dig[i] \
                        and got["ver"][i] == self.want_ver[i]
                else:  # entries of pieces that are not final are left alone
                    ok = ok and got["osize"][i] == FILL * 0x01010101 and (got["dig"][i] == FILL).all() \
                        and got["ver"][i] == FILL
                if not ok:
                    bad.append((c.desc, j, int(got["poff"][i]), int(self.want_poff[i]), int(got["psize"][i]),
                                int(self.want_psize[i]), int(got["osize"][i]), int(self.want_osize[i]),
                                int(got["ver"][i]), self.want_ver[i]))
                i += 1
        assert not bad, bad[:4]
        idx = sorted(self.want_b64)
        want_b64 = M.b64_records([self.want_b64[s] for s in idx], B64_STATE_DTYPE)
        assert got["b64"][idx].tobytes() == want_b64.tobytes(), [
            (s, got["b64"][s], w) for s, w in zip(idx, want_b64) if got["b64"][s].tobytes() != w.tobytes()][:3]
        want_sha = M.sha_records([self.want_sha[s] for s in idx], STATE_DTYPE)
        assert M.sha_records_differ(got["sha"][idx], want_sha) == []
        rest = np.setdiff1d(np.arange(self.n_states), idx)
        assert got["b64"][rest].tobytes() == new_b64_states(rest.size).tobytes()
        assert got["sha"][rest].tobytes() == new_states(rest.size).tobytes()

    def where(self, pos):
        for c in self.chains:
            for k, slot in enumerate(c.slots):
                if slot - 16 <= pos < slot + c.cap + 16:
                    return f"{c.desc}: chunk {k}, slot byte {pos - slot} of {c.cap}"
        return f"arena byte {pos}"

    def check(self):
        """The new launch against the models and against the existing route."""
        seq = self.run_seq()
        self.check_against_models(seq)
        one = self.run_one_per_launch()
        for k in ("b64", "out", "osize", "dig", "ver", "poff", "psize"):
            assert seq[k].tobytes() == one[k].tobytes(), k
        assert M.sha_records_differ(seq["sha"], one["sha"]) == [] and M.sha_records_differ(one["sha"], seq["sha"]) == []
        return seq


def chunk(n, seed=0) -> bytes:
    return W.chunk_bytes(n, seed)


def cut_styles(text: bytes, rng):
    """The ways a text is cut: {name: pieces}."""
    n = len(text)
    mid = n // 2
    return {
        "line ends": cut(text, [73 * k for k in (1, 30, 31, 90)]),
        "mid-group": cut(text, [73 * 10 + 2, 73 * 40 + 4 * 5 + 1, mid // 4 * 4 + 3]),
        "mid-line": cut(text, [73 * 3 + 36, 73 * 50 + 8, 73 * 100 + 72]),
        "one character and empty": cut(text, [0, 1, 2, 2, 3, mid, mid, mid + 1, n - 1, n]),
        "longer than a tile, then tiny": cut(text, [5256 + 700, 5256 + 701, 5256 + 705, 5256 + 705, 5256 + 778]),
        "random": cut(text, rng.integers(0, n + 1, 6)),
        "whole": [text],
    }


def varied_chains(n_chains, rng, first_state=0):
    """Chains of both layouts and every cut style over chunks of two tiles and a
    ragged end, and over the tiny chunks."""
    sizes = [9000, 0, 1, 2, 3, 54, 55, 2 * TILE, 9001, 8999]
    chains = []
    for k in range(n_chains):
        size = sizes[k % len(sizes)] if k % 3 else 9000 - k
        layout = ("xmlrpc", "flat")[(k // 2) % 2]
        data = chunk(size, seed=k)
        text = text_of(data, layout)
        styles = cut_styles(text, rng)
        name = list(styles)[k % len(styles)]
        chains.append(Chain(first_state + k, styles[name], desc=f"chain {k}: {size} B {layout}, cut {name}"))
    return chains


@pytest.mark.parametrize("lines,flat", SWITCHES)
@pytest.mark.parametrize("n_chains", [1, 2, 65])
def test_cuts_layouts_and_switches(switches, lines, flat, n_chains):
    """1, 2 and 65 chains (chains of both layouts in one launch), every cut
    style, all four settings of the line/flat switches."""
    switches(lines, flat)
    rng = np.random.default_rng(100 + n_chains)
    chains = varied_chains(n_chains, rng, first_state=1)
    Scene(chains, n_chains + 2).check()


@pytest.mark.parametrize("lines,flat", [(1, 0), (1, 1), (0, 0)])
def test_damage_in_the_first_a_middle_and_the_last_piece(switches, lines, flat):
    switches(lines, flat)
    chains = []
    for layout in ("xmlrpc", "flat"):
        data = chunk(9000, seed=3)
        text = text_of(data, layout)
        at = [2000, 2001, 7000, 9500]  # five pieces
        edges = [0] + at + [len(text)]
        for kind in ("junk", "eq", "cut", "ins_junk", "drop"):
            for where in (0, 2, 4):
                pos = (edges[where] + edges[where + 1]) // 2 + (1 if kind == "eq" else 0)
                bad = W.damage(text, kind, pos)
                pieces = cut(bad, at)
                # the receiver expects a chunk of the undamaged size: the verdict is 1 only where the damage leaves
                # the decoded length as it was (junk that is skipped)
                c = Chain(len(chains), pieces, cap=len(data), desc=f"{layout} {kind} at {pos} (piece {where})")
                chains.append(c)
    scene = Scene(chains, len(chains))
    got = scene.check()
    i = 0
    for c in scene.chains:
        i += len(c.pieces)
        full = W.decode(b"".join(c.pieces))
        assert got["ver"][i - 1] == (1 if len(full) == c.cap else 0), c.desc


@pytest.mark.parametrize("lines,flat", [(1, 0), (0, 1)])
def test_text_that_decodes_past_the_cap_in_a_middle_piece(switches, lines, flat):
    switches(lines, flat)
    chains = []
    for k, layout in enumerate(("xmlrpc", "flat")):
        text = text_of(chunk(9000, seed=5), layout)
        for cap in (0, 1, 5000, TILE, TILE + 1, 8998):
            pieces = cut(text, [3000, 6000 + k, 9000])
            chains.append(Chain(len(chains), pieces, cap=cap, desc=f"{layout} cap {cap}"))
    got = Scene(chains, len(chains)).check()
    assert not got["ver"][3::4].any() and (got["osize"][3::4] == np.array([c.cap + 1 for c in chains])).all()


def test_a_refused_cap_in_the_middle_of_a_chain(switches):
    """Launch only: a piece whose chunk size is over 1 GiB decodes nothing and
    hands the hash an empty piece, and the chain goes on with the next piece --
    every barrier of the workgroup's loop is still met by all of it.  Refused
    first pieces, refused final pieces and a chain of refused pieces only."""
    switches(1, 1)
    text = text_of(chunk(9000, seed=6), "xmlrpc")
    p = cut(text, [4000, 4100, 8000])
    cap = 9000
    chains = [
        Chain(0, p, caps=[cap, BIG, cap, cap], cap=cap, desc="refused in the middle"),
        Chain(1, p, caps=[BIG, cap, cap, cap], cap=cap, desc="refused first"),
        Chain(2, p, caps=[cap, cap, cap, BIG], cap=cap, desc="refused final"),
        Chain(3, p[:2], caps=[BIG, BIG], finals=[False, False], cap=cap, desc="refused only"),
        Chain(4, p, cap=cap, desc="honest neighbour"),
        Chain(5, p[:3], caps=[cap, BIG, cap], finals=[False, True, False], cap=cap, desc="refused final in mid-run"),
    ]
    got = Scene(chains, 6).check()
    assert got["ver"][3] == 0 and got["ver"][17] == 1  # a skipped piece's text is missing; the neighbour verifies


def test_a_final_in_mid_run_starts_the_next_chunk(switches):
    """Launch only: both records restart in registers and the pieces behind the
    final one begin a new chunk (in a slot of its own: Scene)."""
    switches(1, 0)
    a, b = chunk(5000, seed=7), chunk(4000, seed=8)
    chains = []
    for k, layout in enumerate(("xmlrpc", "flat")):
        ta, tb = text_of(a, layout), text_of(b, layout)
        pieces = cut(ta, [1000, 3001]) + cut(tb, [2000]) + [b"", tb[:100]]
        chains.append(Chain(k, pieces, finals=[0, 0, 1, 0, 1, 1, 0], cap=5000, desc=f"{layout} three chunks and a part"))
    got = Scene(chains, 2).check()
    assert got["osize"][[2, 4, 5]].tolist() == [5000, 4000, 0] and got["ver"][[2, 4, 5]].tolist() == [1, 0, 0]
    assert got["b64"]["decoded"].tolist() == [72, 75]  # 100 characters: 99 of the alphabet in lines, 100 unbroken


def feed_batch(hasher, chains, seq, n_states):
    """The chains through update_text_seq in one call (pieces interleaved round
    by round), or through update_text one piece per chain per call."""
    out_len = max(c.slot + c.cap for c in chains) + 32
    out = np.full(out_len, FILL, dtype=np.uint8)
    b64, sha = new_b64_states(n_states), new_states(n_states)
    rounds = max(len(c.pieces) for c in chains)
    order = [(k, r) for r in range(rounds) for k, c in enumerate(chains) if r < len(c.pieces)]
    results = {}
    calls = [order] if seq else [[(k, r) for k, r in order if r == rr] for rr in range(rounds)]
    for call in calls:
        text = b"".join(chains[k].pieces[r] for k, r in call)
        lens = [len(chains[k].pieces[r]) for k, r in call]
        offs = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
        exp = np.array([np.frombuffer(sha1(W.decode(b"".join(chains[k].pieces))[:chains[k].cap]), dtype=np.uint8)
                        for k, _ in call])
        fn = hasher.update_text_seq if seq else hasher.update_text
        sizes, ver = fn(b64, sha, np.frombuffer(text + b"\0", dtype=np.uint8), offs, lens, out,
                        [chains[k].slot for k, _ in call], [chains[k].cap for k, _ in call],
                        state_of=[chains[k].state for k, _ in call], final=[chains[k].finals[r] for k, r in call],
                        expected=exp)
        for j, kr in enumerate(call):
            results[kr] = (int(sizes[j]), bool(ver[j]))
    return b64, sha, out, results


@pytest.mark.parametrize("lines,flat", SWITCHES)
def test_batch_equals_one_piece_per_call_counters_included(hasher, switches, lines, flat):
    """update_text_seq in one call against update_text fed the same pieces one
    per chain per call: records, bytes, lengths, verdicts and the per-path
    counters (lbf_ctx_b64_update_stats / lbf_ctx_b64_flat_stats)."""
    switches(lines, flat)
    rng = np.random.default_rng(200)
    chains = varied_chains(12, rng)
    Scene(chains, 12)  # assigns the slots
    runs = []
    for seq in (False, True):
        s0, f0 = hasher.b64_update_stats(), hasher.b64_flat_stats()
        b64, sha, out, results = feed_batch(hasher, chains, seq, 12)
        s1, f1 = hasher.b64_update_stats(), hasher.b64_flat_stats()
        counters = (s1["line_chars"] - s0["line_chars"], s1["scan_chars"] - s0["scan_chars"],
                    f1["flat_chars"] - f0["flat_chars"])
        runs.append((b64.tobytes(), sha.tobytes(), out.tobytes(), results, counters))
    assert runs[0][3] == runs[1][3]
    assert runs[0][4] == runs[1][4], (runs[0][4], runs[1][4])
    assert sum(runs[1][4][:2]) == sum(len(p) for c in chains for p in c.pieces)
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1] and runs[0][2] == runs[1][2]
    # and against the reference decode: every chain verified, the arena holds the chunks and nothing else
    want = np.full(len(runs[1][2]), FILL, dtype=np.uint8)
    for k, c in enumerate(chains):
        data = W.decode(b"".join(c.pieces))
        want[c.slot:c.slot + len(data)] = np.frombuffer(data, dtype=np.uint8)
        assert runs[1][3][(k, len(c.pieces) - 1)] == (len(data), True), c.desc
    assert runs[1][2] == want.tobytes()


def test_a_call_without_repeats_equals_update_text(hasher, switches):
    switches(1, 1)
    rng = np.random.default_rng(201)
    chains = [Chain(c.state, [b"".join(c.pieces)], desc=c.desc) for c in varied_chains(9, rng)]
    Scene(chains, 9)
    a = feed_batch(hasher, chains, False, 9)
    b = feed_batch(hasher, chains, True, 9)
    assert a[3] == b[3] and all(x.tobytes() == y.tobytes() for x, y in zip(a[:3], b[:3]))


def test_batch_refusals_leave_everything_untouched(hasher):
    data = chunk(300, seed=9)
    text = np.frombuffer(text_of(data, "xmlrpc") + b"\0", dtype=np.uint8)
    n_text = text.size - 1
    out = np.full(1000, FILL, dtype=np.uint8)

    def call(so, toff, tlen, fin, caps, ooff, b64=None, sha=None):
        b64 = new_b64_states(3) if b64 is None else b64
        sha = new_states(3) if sha is None else sha
        before = (b64.tobytes(), sha.tobytes())
        n = len(so)
        sizes = np.full(n, 0xEEEEEEEE, dtype=np.uint32)
        ver = np.full(n, FILL, dtype=np.uint8)
        a = lambda x, dt: np.ascontiguousarray(x, dtype=dt)  # noqa: E731
        so, toff, tlen, fin, caps, ooff = (a(so, np.uint32), a(toff, np.uint64), a(tlen, np.uint32), a(fin, np.uint8),
                                           a(caps, np.uint32), a(ooff, np.uint64))
        exp = np.zeros((n, 20), dtype=np.uint8)
        rc = _capi.load().lbf_b64_update_seq_batch(
            hasher._h, b64.ctypes.data, sha.ctypes.data, 3, so.ctypes.data, text.ctypes.data, n_text, toff.ctypes.data,
            tlen.ctypes.data, fin.ctypes.data, n, caps.ctypes.data, exp.ctypes.data,
            out.ctypes.data, out.size, ooff.ctypes.data, sizes.ctypes.data, ver.ctypes.data)
        msg = _capi.load().lbf_last_error().decode()
        untouched = ((b64.tobytes(), sha.tobytes()) == before and (out == FILL).all() and (sizes == 0xEEEEEEEE).all()
                     and (ver == FILL).all())
        return rc, msg, untouched

    bad_b64 = new_b64_states(3)
    bad_b64["ncarry"][1] = 4
    cases = [
        ("is final", 0, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[1, 0, 0], caps=[300, 300, 300],
                             ooff=[0, 400, 0])),
        ("another slot", 2, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                 caps=[300, 300, 300], ooff=[0, 400, 1])),
        ("another slot", 2, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                 caps=[300, 300, 299], ooff=[0, 400, 0])),
        ("overlaps", 1, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1], caps=[300, 300, 300],
                             ooff=[0, 299, 0])),
        ("text outside", 2, dict(so=[1, 0, 1], toff=[0, 0, n_text], tlen=[100, 50, 1], fin=[0, 0, 1],
                                 caps=[300, 300, 300], ooff=[0, 400, 0])),
        ("slot outside", 1, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                 caps=[300, 300, 300], ooff=[0, 701, 0])),
        ("names state 3", 1, dict(so=[1, 3, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                  caps=[300, 300, 300], ooff=[0, 400, 0])),
        ("more than 1 GiB", 2, dict(so=[1, 0, 2], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                    caps=[300, 300, BIG], ooff=[0, 400, 0])),
        ("corrupt state", 0, dict(so=[1, 0, 1], toff=[0, 0, 100], tlen=[100, 50, 100], fin=[0, 0, 1],
                                  caps=[300, 300, 300], ooff=[0, 400, 0], b64=bad_b64)),
    ]
    for what, piece, kw in cases:
        rc, msg, untouched = call(**kw)
        assert rc == _capi.LBF_ERR_INVALID and what in msg and f"piece {piece} " in msg, (what, rc, msg)
        assert untouched, what
    # what update_text refuses as "the second piece" is what this call is for
    b64, sha = new_b64_states(3), new_states(3)
    with pytest.raises(LbfError):
        hasher.update_text(b64, sha, text, [0, 100], [100, n_text - 100], out, [0, 0], [300, 300], state_of=[1, 1])
    sizes, ver = hasher.update_text_seq(b64, sha, text, [0, 100], [100, n_text - 100], out, [0, 0], [300, 300],
                                        state_of=[1, 1], final=[0, 1],
                                        expected=np.frombuffer(sha1(data) * 2, dtype=np.uint8))
    assert sizes.tolist() == [0, 300] and ver.tolist() == [False, True]
    assert out[:300].tobytes() == data and (out[300:] == FILL).all()


def test_launch_checks_its_tables():
    """The checks before anything is enqueued: a chain table that does not fit
    its allocation or is misaligned, a missing table."""
    scene = Scene([Chain(0, [b"QUJD"], desc="abc")], 1)
    bufs = scene.upload()
    try:
        def launch(cf, n_chains):
            H.b64_update_seq_launch(bufs["b64"], bufs["sha"], 1, bufs["cs"], cf, n_chains, bufs["text"], bufs["toff"],
                                    bufs["tlen"], bufs["fin"], 1, bufs["out"], bufs["slot"], bufs["cap"],
                                    bufs["osize"], bufs["dig"], bufs["exp"], bufs["ver"], bufs["poff"], bufs["psize"])
        for cf, n_chains, what in ((bufs["cf"], 4, "chain_"), (bufs["cf"].ptr + 2, 1, "aligned"), (None, 1, "null")):
            with pytest.raises(LbfError) as e:
                launch(cf, n_chains)
            assert e.value.status == _capi.LBF_ERR_INVALID and what in str(e.value), str(e.value)
        launch(bufs["cf"], 1)
        H.synchronize()
        assert bufs["out"].download(3, scene.chains[0].slot).tobytes() == b"ABC"
    finally:
        for b in bufs.values():
            b.free()

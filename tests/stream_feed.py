"""Work for eight streams at once, shared by tests/test_gpu_streams.py and the
child process it starts (python -m tests.stream_feed): four streams decode
chunk text piece by piece through lbf_b64_update_launch, two absorb raw bytes
through lbf_sha1_update_launch, two hash through lbf_sha1_uniform_launch, round
chained behind round with the states left on the device and no host wait.

Everything a launch reads is uploaded before the first enqueue and everything
it may write is read back after the last, so what a run must leave behind is
known before it starts: `plan()` works it out once, from tests/wire_layouts.py,
tests/wire_piece_model.py, tests/sha1_model.py, hashlib and the oracle alone,
and no test changes it.  `Run.problems()` then holds the device's bytes against
it: the one arena the four decode streams share (slots touch, neighbours belong
to different streams), both record arrays, every launch's out_sizes, digests
and verdicts (0xEE where a piece is not final), and the gaps between the tables.
"""
import ctypes
import functools
import hashlib
import json
import threading

import numpy as np

from bitflood_amd import B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, _capi, new_b64_states, new_states
from bitflood_amd import hashing as H
from tests import sha1_model
from tests import wire_flat_model as F
from tests import wire_layouts as W
from tests import wire_piece_model as M
from tests.test_gpu_b64_fused import TILE_TEXT, mixed_text
from tests.test_gpu_b64_update import FILL, Chain, _ragged_chains, model_update, sha1
from tests.test_gpu_update import Arena

T = F.TILE_BYTES
DECODERS, UPDATERS, HASHERS = 4, 2, 2
STREAMS = DECODERS + UPDATERS + HASHERS
ROUNDS = 8
PLUG_BYTES = 8 << 20
# (chains, bytes each): auto picks the 64-chain producer/consumer kernel, its two-group form and the LDS-staged one
HASH_SHAPES = ((64, 4099), (16448, 192), (33000, 192))
# (fused, lines, flat): the unfused route with lines, lines + flat and the scan alone, the fused one with
# lines + flat, flat and the scan alone
ROUTES = ((False, True, False), (False, True, True), (False, False, False),
          (True, True, True), (True, False, True), (True, False, False))
E4 = 0xEEEEEEEE


def set_route(route):
    """The three process-wide switches; returns what they were."""
    fused, lines, flat = route
    return H.set_b64_fused(fused), H.set_b64_lines(lines), H.set_b64_flat(flat)


# ------------------------------------------------------------ the decode streams' chains
def _cut(t, cuts):
    cuts = [0] + list(cuts) + [len(t)]
    return [t[a:b] for a, b in zip(cuts, cuts[1:])]


def _unbroken(c, i, rng):
    """Chain i of _ragged_chains as a Java or Perl peer sends it, cut anew into as many pieces."""
    t = F.text(c.want)
    if i % 7 == 0:
        t = W.damage(t, "ins_junk", int(rng.integers(0, len(t) + 1)))
    cuts = sorted(rng.integers(0, len(t) + 1, len(c.pieces) - 1).tolist())
    return Chain(_cut(t, cuts), chunk=c.want, digest_ok=i % 11 != 0, desc=c.desc + ", unbroken")


def _big(s, k, rng):
    """2T + 100 .. 5T + 1000 bytes in three pieces, cut within 80 characters of a tile edge of the layout."""
    size = 2 * T + 100 + k * (3 * T + 900) // 5
    layout = ("xmlrpc", "unbroken", "mixed")[k % 3]
    d = W.chunk_bytes(size, seed=60 + s)
    e1, e2 = (int(x) for x in rng.integers(-80, 81, 2))
    if layout == "mixed":
        p1, p2, p3 = mixed_text(d, k % 4, (k + s) % 4)
        t = p1 + p2 + p3
        cuts = [W.DEC_TEXT + e1, len(p1) + F.TILE_TEXT + e2]  # the line tiles' edge, the flat tiles' edge
    else:
        t = (W.xmlrpc_text if layout == "xmlrpc" else F.text)(d)
        cuts = [TILE_TEXT[layout] + e1, 2 * TILE_TEXT[layout] + e2]
    assert 0 < cuts[0] < cuts[1] < len(t)
    return Chain(_cut(t, cuts), chunk=d, desc=f"{layout} {size} B cut at {cuts}")


def _open(s, k):
    """A chain that never gets its final piece: two pieces, the second ending with (s + k) % 4 sextets carried."""
    nc = (s + k) % 4
    d = W.chunk_bytes(1500 + 211 * k + 17 * s, seed=70)
    t = (W.xmlrpc_text if k % 2 else F.text)(d)
    a = 900 + 100 * k
    while len(model_update(M.init(), t[:a])[0][1]) != nc:
        a += 1
    return Chain([t[:300 + s], t[300 + s:a]], cap=len(d), desc=f"unfinished after {a} characters, {nc} carried")


@functools.lru_cache(maxsize=None)
def decode_chains(s):
    """Stream s's 35 chains and, for each, whether its last piece is the final one."""
    rng = np.random.default_rng(5100 + s)
    ragged = _ragged_chains(24, 8100 + s)
    chains = [c if i % 2 == 0 else _unbroken(c, i, rng) for i, c in enumerate(ragged)]
    assert [c.verdict for c in chains] == [i % 11 != 0 for i in range(24)]
    chains += [_big(s, k, rng) for k in range(6)]
    for k, (cap, delta) in enumerate(((300 + s, 1), (4097 + s, -1))):
        d = W.chunk_bytes(cap + delta, seed=80 + s)
        t = (W.xmlrpc_text if (s + k) % 2 else F.text)(d)
        a = W.b64_len(cap // 3 * 3) if (s + k) % 2 else cap // 3 * 4  # the groups that fit the slot whole
        c = Chain([t[:a // 2], t[a // 2:a], t[a:]], cap=cap, desc=f"cap {cap}, text decodes to {cap + delta}")
        # the digest is that of the slot's bytes: only the length can fail the verdict
        assert not c.verdict and c.expected == sha1(c.want[:cap]) and c.size == (cap + 1 if delta > 0 else cap - 1)
        chains.append(c)
    closed = [True] * len(chains)
    chains += [_open(s, k) for k in range(3)]
    closed += [False] * 3
    assert len(chains) == 35 and max(len(c.pieces) for c in chains) <= ROUNDS
    return tuple(chains), tuple(closed)


# ------------------------------------------------------------ the update streams' chains
@functools.lru_cache(maxsize=None)
def update_chains(u):
    """65 chunks of 0..5,000 bytes, each fed in three to eight calls at random cut
    points (tests/test_gpu_update.py, test_ragged_waves); the last three never
    get their final flag."""
    n = 65
    rng = np.random.default_rng(7100 + u)
    sizes = rng.integers(0, 5001, n)
    chunks = [rng.integers(0, 256, int(s), dtype=np.uint8).tobytes() for s in sizes]
    arena = Arena(phase=3 + 8 * u)
    start = [arena.put(c) for c in chunks]
    calls = rng.integers(3, 9, n)
    cuts = [[0] + sorted(rng.integers(0, int(sizes[c]) + 1, int(calls[c]) - 1).tolist()) + [int(sizes[c])]
            for c in range(n)]
    return chunks, start, arena.buffer(), [int(x) for x in calls], cuts, [c < n - 3 for c in range(n)]


# ------------------------------------------------------------ what a run must leave behind
class Plan:
    """Every table of every launch, and the device's bytes after the last one."""

    def __init__(self):
        self.tables, self.want = {}, {}     # name -> array as uploaded / as it must come back
        self._decoders()
        self._updaters()
        rng = np.random.default_rng(9100)
        self.data = rng.integers(0, 256, PLUG_BYTES, dtype=np.uint8)
        self.plug_digest = hashlib.sha1(self.data.tobytes()).digest()

    def _table(self, name, up, back=None):
        self.tables[name] = np.ascontiguousarray(up)
        self.want[name] = self.tables[name] if back is None else np.ascontiguousarray(back)

    def _decoders(self):
        per = [decode_chains(s) for s in range(DECODERS)]
        n_each = len(per[0][0])
        self.n_states = DECODERS * n_each
        chain = lambda g: per[g % DECODERS][0][g // DECODERS]  # noqa: E731  slots and records go round the streams
        self.slot = np.zeros(self.n_states, dtype=np.uint64)
        pos = 16
        for g in range(self.n_states):
            self.slot[g] = pos
            pos += chain(g).cap
        self.arena = np.full(pos + 16, FILL, dtype=np.uint8)
        self.chain_desc = [f"stream {g % DECODERS}: {chain(g).desc}" for g in range(self.n_states)]
        b64, sha = new_b64_states(self.n_states), new_states(self.n_states)
        want_b64, want_sha = b64.copy(), sha.copy()
        self.live = {}
        for s, (chains, closed) in enumerate(per):
            state, sofar = [M.init()] * n_each, [b""] * n_each
            for r in range(ROUNDS):
                live = [j for j, c in enumerate(chains) if r < len(c.pieces)]
                self.live[s, r] = live
                m = len(live)
                fin = np.array([closed[j] and r == len(chains[j].pieces) - 1 for j in live], dtype=np.uint8)
                parts, toff, at = [], [], 0
                for j in live:  # the pieces one after another, or each at 5 mod 16
                    pad = (5 - at) % 16 if s % 2 else 0
                    parts.append(bytes(pad) + chains[j].pieces[r])
                    toff.append(at + pad)
                    at += len(parts[-1])
                g = np.array([DECODERS * j + s for j in live], dtype=np.uint32)
                osz, ver = np.full(m, E4, dtype=np.uint32), np.full(m, FILL, dtype=np.uint8)
                dig = np.full((m, 20), FILL, dtype=np.uint8)
                for k, j in enumerate(live):
                    c = chains[j]
                    state[j], new = model_update(state[j], c.pieces[r])
                    sofar[j] += new
                    if fin[k]:
                        assert sofar[j] == c.want
                        osz[k], ver[k] = c.size, int(c.verdict)
                        dig[k] = np.frombuffer(sha1(c.want[:c.cap]), dtype=np.uint8)
                key = f"d{s}.{r}."
                self._table(key + "so", g)
                self._table(key + "text", np.frombuffer(b"".join(parts) + b"\0", dtype=np.uint8))
                self._table(key + "toff", np.array(toff, dtype=np.uint64))
                self._table(key + "tlen", np.array([len(chains[j].pieces[r]) for j in live], dtype=np.uint32))
                self._table(key + "fin", fin)
                self._table(key + "ooff", self.slot[g])
                self._table(key + "caps", np.array([chains[j].cap for j in live], dtype=np.uint32))
                self._table(key + "exp", np.frombuffer(b"".join(chains[j].expected for j in live), dtype=np.uint8))
                self._table(key + "osz", np.full(m, E4, dtype=np.uint32), osz)
                self._table(key + "dig", np.full((m, 20), FILL, dtype=np.uint8), dig)
                self._table(key + "ver", np.full(m, FILL, dtype=np.uint8), ver)
            for j, c in enumerate(chains):
                g = DECODERS * j + s
                at, held = int(self.slot[g]), sofar[j][:c.cap]
                self.arena[at:at + len(held)] = np.frombuffer(held, dtype=np.uint8)
                if not closed[j]:  # mid-chunk: the model's records; a chain that has ended is as new
                    want_b64[g] = M.b64_record(state[j])
                    want_sha[g:g + 1] = M.sha_records([M.sha_state(sofar[j], c.cap)], STATE_DTYPE)
        self._table("b64", b64, want_b64)
        # held together by M.sha_records_differ: a block's bytes past `buffered` are free
        self.sha, self.want_sha = sha, want_sha
        self.open = [g for g in range(self.n_states) if not per[g % DECODERS][1][g // DECODERS]]
        assert {int(want_b64["ncarry"][g]) for g in self.open} == {0, 1, 2, 3}

    def _updaters(self):
        self.upd_want_states = []
        for u in range(UPDATERS):
            chunks, start, buf, calls, cuts, closed = update_chains(u)
            n = len(chunks)
            self._table(f"u{u}.data", buf)
            for r in range(ROUNDS):
                live = [c for c in range(n) if calls[c] > r]
                fin = np.array([closed[c] and calls[c] == r + 1 for c in live], dtype=np.uint8)
                want = np.full((len(live), 20), FILL, dtype=np.uint8)
                for k, c in enumerate(live):
                    if fin[k]:
                        want[k] = np.frombuffer(sha1(chunks[c]), dtype=np.uint8)
                key = f"u{u}.{r}."
                self._table(key + "so", np.array(live, dtype=np.uint32))
                self._table(key + "off", np.array([start[c] + cuts[c][r] for c in live], dtype=np.uint64))
                self._table(key + "size", np.array([cuts[c][r + 1] - cuts[c][r] for c in live], dtype=np.uint32))
                self._table(key + "fin", fin)
                self._table(key + "dig", np.full((len(live), 20), FILL, dtype=np.uint8), want)
            states = [sha1_model.init() if closed[c] else sha1_model.update(sha1_model.init(), chunks[c])
                      for c in range(n)]
            self.upd_want_states.append(M.sha_records(states, STATE_DTYPE))
            assert any(int(t) for t in self.upd_want_states[-1]["total"])


@functools.lru_cache(maxsize=None)
def plan():
    p = Plan()
    for a in list(p.tables.values()) + list(p.want.values()) + [p.arena, p.data, p.slot]:
        a.flags.writeable = False
    return p


@functools.lru_cache(maxsize=None)
def hash_want(shape, shift):
    """The oracle's digests of HASH_SHAPES[shape] laid over plan().data from byte `shift`."""
    from tests.oracle_lib import Oracle
    n, size = HASH_SHAPES[shape]
    offs = shift + size * np.arange(n, dtype=np.uint64)
    out = Oracle().sha1_batch(plan().data, offs, np.full(n, size, dtype=np.uint32), nthreads=8)
    out.flags.writeable = False
    return out


# ------------------------------------------------------------ the device side
class Pack:
    """Named arrays side by side in one DeviceBuffer, 256 bytes apart at least and
    0xEE between them: one upload, one download."""

    def __init__(self):
        self.at, self.size = {}, 256
        self.host = []

    def add(self, name, array):
        a = np.ascontiguousarray(array).view(np.uint8).reshape(-1)
        self.at[name] = (self.size, a.size)
        self.host.append((self.size, a))
        self.size += (a.size + 255) // 256 * 256 + 256

    def upload(self):
        blob = np.full(self.size, FILL, dtype=np.uint8)
        self.owned = np.zeros(self.size, dtype=bool)
        for at, a in self.host:
            blob[at:at + a.size] = a
            self.owned[at:at + a.size] = True
        self.dev = DeviceBuffer(self.size)
        self.dev.upload(blob)

    def ptr(self, name):
        return self.dev.ptr + self.at[name][0]

    def download(self):
        self.got = self.dev.download()

    def get(self, name, dtype=np.uint8):
        at, size = self.at[name]
        return self.got[at:at + size].view(dtype)


class Run:
    """One run of the plan: its buffers, its eight streams, the enqueue calls and the check.
    hash_keys names the hash launches the run will make: key -> (shape, shift)."""

    def __init__(self, hash_keys):
        self.plan, self.hash_keys = plan(), dict(hash_keys)
        p, lib = self.plan, _capi.load()
        self.pack = Pack()
        for name, a in p.tables.items():
            self.pack.add(name, a)
        self.pack.add("sha", p.sha)
        for u in range(UPDATERS):
            self.pack.add(f"u{u}.states", new_states(len(update_chains(u)[0])))
        for s in range(DECODERS):
            for r in range(ROUNDS):
                # the piece table a launch hands from its decode to its hash: zeros, so that a hash that ran ahead
                # of its decode would absorb nothing (and give a wrong digest), never read outside the arena
                self.pack.add(f"d{s}.{r}.poff", np.zeros(len(p.live[s, r]), dtype=np.uint64))
                self.pack.add(f"d{s}.{r}.psz", np.zeros(len(p.live[s, r]), dtype=np.uint32))
        for key, (shape, _) in self.hash_keys.items():
            self.pack.add(f"h{key}", np.full(20 * HASH_SHAPES[shape][0], FILL, dtype=np.uint8))
        for q in range(STREAMS):
            self.pack.add(f"plug{q}", np.full(20, FILL, dtype=np.uint8))
        self.pack.upload()
        self.arena = DeviceBuffer(p.arena.size)
        self.arena.upload(np.full(p.arena.size, FILL, dtype=np.uint8))
        self.data = DeviceBuffer(p.data.size)
        self.data.upload(p.data)
        self.streams, self.plugged = [], set()
        for _ in range(STREAMS):
            st = ctypes.c_void_p()
            _capi.check(lib.lbf_stream_create(ctypes.byref(st)))
            self.streams.append(st)
        H.synchronize()

    def close(self):
        lib = _capi.load()
        for st in self.streams:
            _capi.check(lib.lbf_stream_synchronize(st))
        for st in self.streams:
            _capi.check(lib.lbf_stream_destroy(st))
        for b in (self.pack.dev, self.arena, self.data):
            b.free()

    # -- enqueue: nothing here waits for the device
    def plug(self, q):
        """One chain of 8 MiB at the head of stream q: what is enqueued on q behind it waits about 0.1 s."""
        H.uniform_launch(self.data, PLUG_BYTES, PLUG_BYTES, 0, 1, self.pack.ptr(f"plug{q}"), stream=self.streams[q])
        self.plugged.add(q)

    def decode(self, s, r, q=None):
        m = len(self.plan.live[s, r])
        if m == 0:
            return
        t = lambda name: self.pack.ptr(f"d{s}.{r}.{name}")  # noqa: E731
        H.b64_update_launch(self.pack.ptr("b64"), self.pack.ptr("sha"), self.plan.n_states, t("so"), t("text"),
                            t("toff"), t("tlen"), t("fin"), m, self.arena, t("ooff"), t("caps"), t("osz"), t("dig"),
                            t("exp"), t("ver"), t("poff"), t("psz"), stream=self.streams[s if q is None else q])

    def update(self, u, r, q):
        m = self.plan.tables[f"u{u}.{r}.so"].size
        if m == 0:
            return
        t = lambda name: self.pack.ptr(f"u{u}.{r}.{name}")  # noqa: E731
        H.update_launch(self.pack.ptr(f"u{u}.states"), len(update_chains(u)[0]), t("so"), self.pack.ptr(f"u{u}.data"),
                        t("off"), t("size"), t("fin"), m, t("dig"), stream=self.streams[q])

    def hash(self, key, q):
        shape, shift = self.hash_keys[key]
        n, size = HASH_SHAPES[shape]
        H.uniform_launch(self.data.ptr + shift, n * size, size, 0, n, self.pack.ptr(f"h{key}"), stream=self.streams[q])

    # -- the check
    def problems(self):
        """Wait for every stream once, read everything back, and say what differs from the plan."""
        p, lib, bad = self.plan, _capi.load(), []
        for st in self.streams:
            _capi.check(lib.lbf_stream_synchronize(st))
        self.pack.download()
        arena = self.arena.download(p.arena.size)
        wrong = np.flatnonzero(arena != p.arena)
        if wrong.size:
            at = int(wrong[0])
            g = max(int(np.searchsorted(p.slot, at, side="right")) - 1, 0)
            bad.append(f"arena: {wrong.size} bytes differ, the first is byte {at} = slot {g} + {at - int(p.slot[g])} "
                       f"({p.chain_desc[g]}): got {arena[at]:#04x}, want {p.arena[at]:#04x}")
        for s in range(DECODERS):
            for r in range(ROUNDS):
                for name, dt in (("osz", np.uint32), ("dig", np.uint8), ("ver", np.uint8)):
                    key = f"d{s}.{r}.{name}"
                    got, want = self.pack.get(key, dt), p.want[key].reshape(-1)
                    if name == "dig":
                        got, want = got.reshape(-1, 20), want.reshape(-1, 20)
                    for k in np.flatnonzero((got != want).reshape(len(p.live[s, r]), -1).any(axis=1))[:3]:
                        g = DECODERS * p.live[s, r][int(k)] + s
                        bad.append(f"{key}[{k}] ({p.chain_desc[g]}): got {got[k].tolist()}, want {want[k].tolist()}")
        got = self.pack.get("b64", B64_STATE_DTYPE)
        for g in np.flatnonzero(got.view(np.uint8).reshape(-1, 16) != p.want["b64"].view(np.uint8).reshape(-1, 16))[:3]:
            g = int(g) // 16
            bad.append(f"b64 record {g} ({p.chain_desc[g]}): got {got[g]}, want {p.want['b64'][g]}")
        got = self.pack.get("sha", STATE_DTYPE)
        for g in M.sha_records_differ(got, p.want_sha)[:3]:
            bad.append(f"sha record {g} ({p.chain_desc[g]}): got {got[g]}, want {p.want_sha[g]}")
        ended = [g for g in range(p.n_states) if g not in p.open]
        if got[ended].tobytes() != new_states(len(ended)).tobytes():
            bad.append("sha records: a chain that has ended is not as new")
        for u in range(UPDATERS):
            for r in range(ROUNDS):
                key = f"u{u}.{r}.dig"
                got, want = self.pack.get(key).reshape(-1, 20), p.want[key].reshape(-1, 20)
                for k in np.flatnonzero((got != want).any(axis=1))[:3]:
                    bad.append(f"{key}[{k}]: got {bytes(got[k]).hex()}, want {bytes(want[k]).hex()}")
            got, want = self.pack.get(f"u{u}.states", STATE_DTYPE), p.upd_want_states[u]
            for c in M.sha_records_differ(got, want)[:3]:
                bad.append(f"update stream {u}, state {c}: got {got[c]}, want {want[c]}")
            closed = np.array(update_chains(u)[5])
            if got[closed].tobytes() != new_states(int(closed.sum())).tobytes():
                bad.append(f"update stream {u}: a chain that has ended is not as new")
        for key, (shape, shift) in self.hash_keys.items():
            got, want = self.pack.get(f"h{key}").reshape(-1, 20), hash_want(shape, shift)
            diff = np.flatnonzero((got != want).any(axis=1))
            if diff.size:
                bad.append(f"hash launch {key} ({HASH_SHAPES[shape]}): {diff.size} digests differ, the first is "
                           f"{int(diff[0])}")
        for q in range(STREAMS):
            if self.pack.get(f"plug{q}").tobytes() != (p.plug_digest if q in self.plugged else bytes([FILL]) * 20):
                bad.append(f"plug of stream {q}: got {self.pack.get(f'plug{q}').tobytes().hex()}")
        # inputs as uploaded, and 0xEE still between the tables
        for name, a in p.tables.items():
            if p.want[name] is a and name != "b64" and self.pack.get(name).tobytes() != a.tobytes():
                bad.append(f"input table {name} was written")
        if (self.pack.got[~self.pack.owned] != FILL).any():
            at = int(np.flatnonzero((self.pack.got != FILL) & ~self.pack.owned)[0])
            bad.append(f"a byte between the tables was written: byte {at} of the pack")
        return bad


# ------------------------------------------------------------ the two ways to enqueue
def one_thread_hash_keys():
    return {r: (r % 3, r) for r in range(ROUNDS)}


def enqueue_from_one_thread(run, route_of=None):
    """Round by round over the eight streams; route_of(r, s) sets the switches before decode stream s's launch."""
    for q in range(STREAMS):
        run.plug(q)
    for r in range(ROUNDS):
        for s in range(DECODERS):
            if route_of is not None:
                set_route(route_of(r, s))
            run.decode(s, r)
        for u in range(UPDATERS):
            run.update(u, r, DECODERS + u)
        run.hash(r, DECODERS + UPDATERS + r % HASHERS)


def four_thread_hash_keys():
    return {f"{s}.{r}": ((r + s) % 3, 4 * r + s) for s in range(DECODERS) for r in range(ROUNDS)}


def enqueue_from_four_threads(run):
    """Thread s owns stream s and puts all of its work there, round behind round: its plug, its decode launches,
    a hash launch after each, and (threads 0 and 1) an update stream's launches.  The four start together."""
    gate = threading.Barrier(DECODERS)
    errors = []

    def caller(s):
        try:
            gate.wait(timeout=60)
            run.plug(s)
            for r in range(ROUNDS):
                run.decode(s, r)
                if s < UPDATERS:
                    run.update(s, r, s)
                run.hash(f"{s}.{r}", s)
        except BaseException as e:  # collected, reported by the caller
            errors.append(f"thread {s}: {e!r}")

    th = [threading.Thread(target=caller, args=(s,), daemon=True) for s in range(DECODERS)]
    for x in th:
        x.start()
    for x in th:
        x.join(timeout=120)
    if any(x.is_alive() for x in th):
        errors.append("an enqueueing thread did not finish")
    return errors


def four_threads():
    """The whole of the four-thread run: what went wrong, as a list of strings."""
    run = Run(four_thread_hash_keys())
    errors = enqueue_from_four_threads(run)
    if any("did not finish" in e for e in errors):
        return errors  # nothing more is started behind a stuck call, and its buffers stay
    try:
        return errors + run.problems()
    finally:
        run.close()


if __name__ == "__main__":
    found = four_threads()
    print(json.dumps({"problems": found[:10], "count": len(found), "launches": DECODERS * ROUNDS}))

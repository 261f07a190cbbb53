"""Random scenes for the piecewise and one-shot launch calls, with everything
the calls must give -- TEST INFRASTRUCTURE.  No GPU, no pytest, no bitflood_amd.

`case(seed)` is one scene, the same for a seed every time: the input arena, the
size of the 0xEE-filled output arena, the state arrays' length and a list of
calls.  A call names its route (one of ROUTES), the (lines, flat, fused)
switches where the route reads them, its pieces in caller order and `want`:
what the call must leave behind.  Expectations come from hashlib,
tests/sha1_model.py, tests/wire_layouts.py (decode, xmlrpc_text, damage,
KINDS), tests/wire_piece_model.py and tests/wire_encode_model.py; nothing comes
from a GPU path.  `check(scene, k, got)` holds a result against call k's
expectation and raises Mismatch naming the seed, the call, the route, the
switches, the chain and the place, with the line that replays the case.

Only inputs the C ABI's contract allows are drawn (include/lbf_hash.h): offsets
inside their arenas, slots apart from one another, at most one piece per chain
in the one-piece calls, a final piece last among its chain's pieces of a call.
The records a call resumes are the ones the call before it left (the driver,
tests/piece_driver.py, carries them as bytes); none is forged, and no refused
argument is drawn: the features' own tests hold those.

The families, by seed % 4: hash (lbf_sha1_update_*), text (lbf_b64_update_*),
seed (lbf_b64_encode_update_*), shot (lbf_b64_verify_launch /
lbf_verify_encode_b64_launch).  tests/test_piece_cases.py proves on the CPU what
SLICE reaches; tests/test_gpu_piece_fuzz.py runs SLICE on the GPU;
tools/fuzz_pieces.py draws fresh seeds.

The chaining value of an unfinished SHA-1 chain is checked through
tests/sha1_model.py, which is slow (about 7,500 blocks a second): a scene
follows it for H_BUDGET bytes, first come first served, and GROUP scenes make a
pytest test, 512 KiB at the most.  Chains past the budget are still held to the
record's other fields and, when they end, to hashlib's digest.
"""
import base64
import hashlib

import numpy as np

from tests import sha1_model
from tests import wire_encode_model as E
from tests import wire_layouts as W
from tests import wire_piece_model as M

FILL = 0xEE
FILL32 = 0xEEEEEEEE
UINT32_MAX = 0xFFFFFFFF
EMPTY_SHA = hashlib.sha1(b"").digest()
GROUP = 8                      # scenes per pytest test
H_BUDGET = (512 << 10) // GROUP  # bytes of a scene whose intermediate h is model-checked

FAMILIES = ("hash", "text", "seed", "shot")
ROUTES = {"hash": ("update_chunks", "update_chunks_seq", "update_launch", "update_seq_launch"),
          "text": ("update_text", "update_text_seq", "b64_update_launch", "b64_update_seq_launch"),
          "seed": ("update_encode", "b64_encode_update_launch"),
          "shot": ("verify_b64_launch", "verify_encode_b64_launch")}
HOST = {"update_chunks", "update_chunks_seq", "update_text", "update_text_seq", "update_encode"}
SEQ = {"update_chunks_seq", "update_seq_launch", "update_text_seq", "b64_update_seq_launch"}
LAYOUTS = ("xmlrpc", "flat")
SIZE_CLASSES = ("0", "1-2", "3-53", "54-55", "tile", "3887-3889", "wg+")
CAP_RELATIONS = ("equal", "shorter", "longer")
PER_PIECE = ("out_sizes", "text_sizes", "new_offsets", "new_lens", "verdicts", "digests")
B64_FIELDS = ("decoded", "carry", "ncarry", "ended", "zero")
ENC_FIELDS = ("taken", "carry", "ncarry", "layout", "zero")
SHA_INIT = (tuple(sha1_model.H0), 0, 0, b"")

# The fixed slice: the seeds tests/test_piece_cases.py counts its ledger over and
# tests/test_gpu_piece_fuzz.py runs, GROUP to a test.  seed % 4 is the family.
SLICE = {
    "hash": tuple(range(0, 160, 4)),
    "text": tuple(range(1, 416, 4)),
    "seed": tuple(range(2, 160, 4)),
    "shot": tuple(range(3, 64, 4)),
}


class Mismatch(AssertionError):
    pass


class Call:
    """One call.  Per piece, in caller order: chain (index into scene.chains),
    state_of, src_off / src_len (the piece in the input arena), final, expected
    (20 bytes), dst_off / cap (the chain's slot in the output arena)."""

    def __init__(self, route, switches=None, fresh=False, **opts):
        self.route, self.switches, self.fresh, self.opts = route, switches, fresh, opts
        self.chain, self.state_of, self.src_off, self.src_len, self.final = [], [], [], [], []
        self.expected, self.dst_off, self.cap = [], [], []
        self.want = {}

    @property
    def n(self):
        return len(self.chain)

    def add(self, chain, state, src_off, src_len, final, expected, dst_off=0, cap=0):
        for lst, v in ((self.chain, chain), (self.state_of, state), (self.src_off, src_off), (self.src_len, src_len),
                       (self.final, 1 if final else 0), (self.expected, bytes(expected)), (self.dst_off, dst_off),
                       (self.cap, cap)):
            lst.append(v)

    def expected_array(self):
        return np.frombuffer(b"".join(self.expected), dtype=np.uint8).reshape(-1, 20).copy()


class Scene:
    def __init__(self, seed, family):
        self.seed, self.family = seed, family
        self.src = bytearray()
        self.dst_len, self.n_states = 0, 0
        self.chains, self.calls = [], []   # chains: dicts (desc, layout, ...; "visits": [(call, route, switches, pending)])
        self.slots = []                    # (start, length, chain) in the output arena
        self.h_left = H_BUDGET
        self.enc_layouts = None            # seed family: the layout of every state's record

    def place(self, data: bytes, phase: int) -> int:
        """Append `data` to the input arena at `phase` mod 16, a byte at least from what lies in front."""
        pos = len(self.src) + 1
        pos += (phase - pos) % 16
        self.src += bytes([FILL]) * (pos - len(self.src))
        self.src += data
        return pos

    def slot(self, length: int, phase: int, chain: int) -> int:
        pos = self.dst_len + 3
        pos += (phase - pos) % 16
        self.dst_len = pos + length
        self.slots.append((pos, length, chain))
        return pos

    def where(self, pos: int) -> str:
        for start, length, chain in self.slots:
            if start <= pos < start + length:
                return f"byte {pos - start} of the {length}-byte slot of chain {chain}: {self.chains[chain]['desc']}"
        near = min(self.slots, key=lambda s: min(abs(pos - s[0]), abs(pos - s[0] - s[1])), default=None)
        return "outside every slot" + (f" (nearest: chain {near[2]}'s at {near[0]}, {near[1]} bytes)" if near else "")

    def describe(self, k: int, place: str, chain=None) -> str:
        call = self.calls[k]
        sw = "" if call.switches is None else " (lines, flat, fused) = %d%d%d" % call.switches
        who = "" if chain is None else f"\n  chain {chain}: {self.chains[chain]['desc']}"
        replay = f"\n  replay: python tools/fuzz_pieces.py --seed {self.seed} --cases 1" if isinstance(self.seed, int) else ""
        return (f"seed {self.seed} ({self.family}) call {k} of {len(self.calls)} route {call.route}{sw} {call.opts or ''}: "
                f"{place}{who}{replay}")


class _Sha:
    """The SHA-1 record of one chain by the data alone; h through the model while the scene's budget lasts."""

    def __init__(self, scene):
        self.scene = scene
        self.reset()

    def reset(self):
        self.h, self.total, self.block, self.absorbed = list(sha1_model.H0), 0, b"", bytearray()

    def absorb(self, data: bytes):
        self.absorbed += data
        data = self.block + bytes(data)
        full = len(data) // 64 * 64
        if full and self.h is not None:
            if self.scene.h_left >= full:
                self.scene.h_left -= full
                for p in range(0, full, 64):
                    self.h = sha1_model.compress(self.h, data[p:p + 64])
            else:
                self.h = None
        self.total += len(data) - len(self.block)
        self.block = data[full:]

    def digest(self) -> bytes:
        return hashlib.sha1(bytes(self.absorbed)).digest()

    def record(self):
        return (None if self.h is None else tuple(self.h), self.total, len(self.block), self.block)


def _wrong(rng, digest: bytes, p=0.1):
    """(expected digest, the 32-bit word made wrong or None): about a tenth are wrong at a random byte and bit."""
    if rng.random() >= p:
        return digest, None
    byte, bit = int(rng.integers(0, 20)), int(rng.integers(0, 8))
    d = bytearray(digest)
    d[byte] ^= 1 << bit
    return bytes(d), byte // 4


def _rand(rng, n: int) -> bytes:
    return rng.integers(0, 256, n, dtype=np.uint8).tobytes()


def _schedule(rng, routes, pieces_of, unfinished=0.15, all_first=False):
    """Which pieces of which chain go into which call: [[(chain, piece)]] per
    call, a chain's pieces in order over the calls and inside a call; the
    one-piece routes get at most one piece of a chain.  Some chains are left
    unfinished; with all_first every chain is in the first call."""
    at = [0] * len(pieces_of)
    stop = [n if rng.random() >= unfinished else int(rng.integers(0, n + 1)) for n in pieces_of]
    stop[0] = max(stop[0], 1)  # a scene has a call
    if all_first:
        stop = [max(x, 1) for x in stop]
    plan = []
    for k, route in enumerate(routes):
        last = k == len(routes) - 1
        dense = rng.random() < 0.35 or (all_first and k == 0)  # every chain that has a piece left is in this call
        take = []
        for c, n in enumerate(pieces_of):
            left = stop[c] - at[c]
            if route in SEQ:
                t = left if last and rng.random() < 0.7 else int(rng.integers(1 if last else 0, 4))
            else:
                t = int(rng.integers(0, 2)) if not last else 1
            take.append(min(max(t, 1) if dense else t, left))
        order, left = [], take[:]
        live = [c for c in range(len(take)) if left[c]]
        while live:  # a random merge that keeps each chain's order
            j = int(rng.integers(0, len(live)))
            c = live[j]
            order.append((c, at[c]))
            at[c] += 1
            left[c] -= 1
            if not left[c]:
                live.pop(j)
        plan.append(order)
    return plan


def _finish(call, want_lists):
    dt = {"out_sizes": np.uint32, "text_sizes": np.uint32, "new_lens": np.uint32, "new_offsets": np.uint64,
          "verdicts": np.uint8}
    for key, vals in want_lists.items():
        if key == "digests":
            call.want[key] = np.frombuffer(b"".join(vals), dtype=np.uint8).reshape(-1, 20).copy()
        else:
            call.want[key] = np.array(vals, dtype=dt[key])


# ------------------------------------------------------------------------- hash
def _hash_piece_size(rng, buffered: int) -> int:
    need = 64 - buffered
    kind = int(rng.integers(0, 5))
    if kind == 0:
        return int(rng.integers(0, need))                       # leaves the block short (an empty piece too)
    if kind == 1:
        return need                                             # tops it up exactly
    if kind == 2:
        return need + int(rng.integers(1, 130))                 # more than it needs
    if kind == 3:
        return (56 + int(rng.integers(0, 8)) - buffered) % 64 + 64 * int(rng.integers(0, 2))  # 56..63 left buffered
    return int(rng.integers(65, 3000))


def _hash_scene(sc, rng):
    n = [1, int(rng.integers(2, 64)), 64, int(rng.integers(65, 129)), int(rng.integers(129, 133))][int(rng.integers(0, 5))]
    sc.n_states = n + int(rng.integers(0, 4))
    states = rng.permutation(sc.n_states)[:n]
    routes = [ROUTES["hash"][int(rng.integers(0, 4))] for _ in range(int(rng.integers(1, 6)))]
    datas = []
    for c in range(n):
        sizes, b = [], 0
        for _ in range(int(rng.integers(1, 7))):
            s = _hash_piece_size(rng, b)
            sizes.append(s)
            b = (b + s) % 64
        datas.append([_rand(rng, s) for s in sizes])
        sc.chains.append({"desc": f"state {int(states[c])}, pieces of {sizes} bytes", "visits": [], "wrong_word": None,
                          "sphases": []})
    plan = _schedule(rng, routes, [len(d) for d in datas], all_first=rng.random() < 0.5)
    sha = [_Sha(sc) for _ in range(n)]
    records = [SHA_INIT] * sc.n_states
    for route, order in zip(routes, plan):
        if not order:
            continue
        k = len(sc.calls)
        verify = bool(rng.integers(0, 2))  # the host calls give digests or verdicts
        call = Call(route, verify=verify) if route in HOST else Call(route)
        keep = 0 if route in HOST else FILL
        dig, ver = [], []
        seen = set()
        for c, p in order:
            ch, data = sc.chains[c], datas[c][p]
            if c not in seen:
                seen.add(c)
                ch["visits"].append((k, route, None, len(sha[c].block)))
            phase = int(rng.integers(0, 16))
            ch["sphases"].append(phase)
            off = sc.place(data, phase)
            final = p == len(datas[c]) - 1
            sha[c].absorb(data)
            exp = bytes(20)
            if final:
                d = sha[c].digest()
                exp, word = _wrong(rng, d)
                if word is not None:
                    ch["wrong_word"] = word
                dig.append(d)
                ver.append(1 if exp == d else 0)
                sha[c].reset()
            else:
                dig.append(bytes([keep]) * 20)
                ver.append(keep)
            call.add(c, int(states[c]), off, len(data), final, exp)
        for c in seen:
            records[int(states[c])] = sha[c].record()
        if route in HOST:
            _finish(call, {"verdicts": ver} if verify else {"digests": dig})
        else:
            _finish(call, {"verdicts": ver, "digests": dig})
        call.want["sha"] = list(records)
        sc.calls.append(call)


# ------------------------------------------------------------------------- text
def _draw_size(rng, cls: int) -> int:
    return [0, int(rng.integers(1, 3)), int(rng.integers(3, 54)), int(rng.integers(54, 56)), int(rng.integers(56, 3887)),
            int(rng.integers(3887, 3890)), int(rng.integers(15553, 20000))][cls]


def text_of(data: bytes, layout: str) -> bytes:
    return W.xmlrpc_text(data) if layout == "xmlrpc" else base64.b64encode(data)


def _cut(text: bytes, edges):
    e = [0] + [min(int(a), len(text)) for a in edges] + [len(text)]
    return [text[a:b] for a, b in zip(e[:-1], e[1:])]


def _damaged(rng, text: bytes, edges):
    """(text, (kind, where, piece) or None): one of W.KINDS in the first, a middle or the last piece of the cutting."""
    if rng.random() >= 0.45:
        return text, None
    e = [0] + list(edges) + [len(text)]
    np_ = len(e) - 1
    where = ("first", "middle", "last")[int(rng.integers(0, 3))]
    if where == "middle" and np_ < 3:
        where = ("first", "last")[int(rng.integers(0, 2))]
    j = 0 if where == "first" else np_ - 1 if where == "last" else int(rng.integers(1, np_ - 1))
    a, b = e[j], e[j + 1]
    kind = W.KINDS[int(rng.integers(0, len(W.KINDS)))]
    inserts = kind == "cut" or kind.startswith("ins_")
    if a == b and not inserts:
        return text, None
    pos = int(rng.integers(a, b + 1)) if inserts and a == b else int(rng.integers(a, b))
    return W.damage(text, kind, pos), (kind, where, j)


def _text_chain(sc, rng, c, state, big_left):
    cls = int(rng.integers(0, 7))
    if cls == 6 and not big_left:
        cls = 4
    size = _draw_size(rng, cls)
    layout = LAYOUTS[int(rng.integers(0, 2))]
    data = _rand(rng, size)
    clean = text_of(data, layout)
    npieces = int(rng.integers(1, 9))
    edges = sorted(int(x) for x in rng.integers(0, len(clean) + 1, npieces - 1))
    text, dmg = _damaged(rng, clean, edges)
    pieces = _cut(text, edges)
    decoded = W.decode(text)
    rel = CAP_RELATIONS[int(rng.integers(0, 3))] if rng.random() < 0.5 else "equal"
    L = len(decoded)
    if rel == "shorter" and L == 0:
        rel = "equal"
    cap = L if rel == "equal" else int(rng.integers(0, L)) if rel == "shorter" else L + int(rng.integers(1, 40))
    sphase = int(rng.integers(0, 16))
    ch = {"desc": f"state {state}, {size} B {layout}, damage {dmg}, {len(pieces)} pieces of {[len(p) for p in pieces]} "
                  f"characters, decodes to {L}, cap {cap} ({rel})",
          "layout": layout, "size_class": SIZE_CLASSES[cls], "cap_rel": rel, "damage": dmg, "visits": [], "wrong_word": None,
          "sphase": sphase, "tphases": [], "cap": cap, "slot": sc.slot(cap, sphase, c), "data": data, "text": text, "fed": 0,
          "pieces": pieces, "decoded": decoded}
    sc.chains.append(ch)
    return cls == 6


def _text_scene(sc, rng):
    n = [1, int(rng.integers(2, 8)), int(rng.integers(8, 24))][int(rng.integers(0, 3))]
    sc.n_states = n + int(rng.integers(0, 3))
    states = rng.permutation(sc.n_states)[:n]
    big = 3
    for c in range(n):
        big -= _text_chain(sc, rng, c, int(states[c]), big > 0)
    routes = [ROUTES["text"][int(rng.integers(0, 4))] for _ in range(int(rng.integers(1, 7)))]
    plan = _schedule(rng, routes, [len(ch["pieces"]) for ch in sc.chains])
    sha = [_Sha(sc) for _ in range(n)]
    dec = [M.init() for _ in range(n)]
    sofar = [b"" for _ in range(n)]
    b64_rec = [M.b64_record(M.init())] * sc.n_states
    sha_rec = [SHA_INIT] * sc.n_states
    arena = np.full(sc.dst_len + 19, FILL, dtype=np.uint8)
    sc.dst_len = arena.size
    for route, order in zip(routes, plan):
        if not order:
            continue
        k = len(sc.calls)
        sw = tuple(int(x) for x in rng.integers(0, 2, 3))
        call = Call(route, switches=sw)
        keep = 0 if route in HOST else FILL
        keep32 = 0 if route in HOST else FILL32
        osz, dig, ver = [], [], []
        seen = set()
        for c, p in order:
            ch, piece = sc.chains[c], sc.chains[c]["pieces"][p]
            if c not in seen:
                seen.add(c)
                ch["visits"].append((k, route, sw, len(dec[c][1])))
            phase = int(rng.integers(0, 16))
            ch["tphases"].append(phase)
            off = sc.place(piece, phase)
            final = p == len(ch["pieces"]) - 1
            cap, slot = ch["cap"], ch["slot"]
            ch["fed"] = p + 1
            before = len(sofar[c])
            dec[c], new = M.update(dec[c], piece)
            sofar[c] += new
            lo, hi = min(before, cap), min(len(sofar[c]), cap)
            arena[slot + lo:slot + hi] = np.frombuffer(sofar[c][lo:hi], dtype=np.uint8)
            sha[c].absorb(sofar[c][lo:hi])
            exp = bytes(20)
            if final:
                d = sha[c].digest()
                exp, word = _wrong(rng, hashlib.sha1(ch["data"]).digest())
                size = len(sofar[c]) if len(sofar[c]) <= cap else cap + 1
                if word is not None and size == cap and sofar[c] == ch["data"]:
                    ch["wrong_word"] = word  # nothing but this bit keeps the verdict from 1
                osz.append(size)
                dig.append(d)
                ver.append(1 if size == cap and d == exp else 0)
                assert sofar[c] == ch["decoded"]
                sha[c].reset()
                dec[c], sofar[c] = M.init(), b""
            else:
                osz.append(keep32)
                dig.append(bytes([keep]) * 20)
                ver.append(keep)
            call.add(c, int(states[c]), off, len(piece), final, exp, slot, cap)
        for c in seen:
            b64_rec[int(states[c])] = M.b64_record(dec[c])
            sha_rec[int(states[c])] = sha[c].record()
        lists = {"out_sizes": osz, "verdicts": ver}
        if route not in HOST:
            lists["digests"] = dig
        _finish(call, lists)
        call.want.update(arena=arena.copy(), rec=list(b64_rec), sha=list(sha_rec))
        sc.calls.append(call)


# ------------------------------------------------------------------------- seed
SEED_SIZES = ((0, 1), (1, 3), (3, 54), (54, 200), (E.TILE_BYTES - 3, E.TILE_BYTES + 4), (2 * E.TILE_BYTES + 1, 15000))
TEXT_CAPS = ("exact", "one short", "zero")


def _seed_scene(sc, rng):
    n = [1, int(rng.integers(2, 8)), int(rng.integers(8, 40))][int(rng.integers(0, 3))]
    sc.n_states = n + int(rng.integers(0, 3))
    states = rng.permutation(sc.n_states)[:n]
    sc.enc_layouts = [int(rng.integers(0, 2)) for _ in range(sc.n_states)]
    datas = []
    for c in range(n):
        layout = sc.enc_layouts[int(states[c])]
        lo, hi = SEED_SIZES[int(rng.integers(0, len(SEED_SIZES) - (1 if c > 6 else 0)))]
        size = int(rng.integers(lo, hi))
        data = _rand(rng, size)
        npieces = int(rng.integers(1, 7))
        edges = sorted(int(x) for x in rng.integers(0, size + 1, npieces - 1))
        datas.append(_cut(data, edges))
        tl = E.text_length(size, layout)
        rel = TEXT_CAPS[int(rng.integers(0, 3))] if rng.random() < 0.4 else "exact"
        if tl == 0:
            rel = "exact"
        cap = tl if rel == "exact" else tl - 1 if rel == "one short" else 0
        sphase = int(rng.integers(0, 16))
        sc.chains.append({"desc": f"state {int(states[c])}, {size} B {LAYOUTS[layout]}, pieces of {[len(p) for p in datas[c]]}"
                                  f" bytes, text {tl}, cap {cap} ({rel})",
                          "layout": LAYOUTS[layout], "cap_rel": rel, "visits": [], "wrong_word": None, "sphase": sphase,
                          "sphases": [], "cap": cap, "slot": sc.slot(cap, sphase, c), "data": data})
    routes = [ROUTES["seed"][int(rng.integers(0, 2))] for _ in range(int(rng.integers(1, 8)))]
    plan = _schedule(rng, routes, [len(d) for d in datas])
    sha = [_Sha(sc) for _ in range(n)]
    enc = [E.init(sc.enc_layouts[int(states[c])]) for c in range(n)]
    enc_rec = [E.record(E.init(lay)) for lay in sc.enc_layouts]
    sha_rec = [SHA_INIT] * sc.n_states
    arena = np.full(sc.dst_len + 19, FILL, dtype=np.uint8)
    sc.dst_len = arena.size
    for route, order in zip(routes, plan):
        if not order:
            continue
        k = len(sc.calls)
        call = Call(route)
        keep = 0 if route in HOST else FILL
        keep32 = 0 if route in HOST else FILL32
        noff, nlen, tsz, dig, ver = [], [], [], [], []
        for c, p in order:
            ch, piece = sc.chains[c], datas[c][p]
            ch["visits"].append((k, route, None, enc[c][0] % 3))
            phase = int(rng.integers(0, 16))
            ch["sphases"].append(phase)
            off = sc.place(piece, phase)
            final = p == len(datas[c]) - 1
            cap, slot = ch["cap"], ch["slot"]
            enc[c], at, chars, tlen = E.update(enc[c], piece, final)
            lo, kept = E.clip(at, chars, cap)
            arena[slot + lo:slot + lo + len(kept)] = np.frombuffer(kept, dtype=np.uint8)
            noff.append(slot + lo)
            nlen.append(len(kept))
            sha[c].absorb(piece)
            exp = bytes(20)
            if final:
                d = sha[c].digest()
                exp, word = _wrong(rng, d, 0.2)
                if word is not None and tlen <= cap:
                    ch["wrong_word"] = word  # nothing but this bit keeps the verdict from 1
                tsz.append(tlen if tlen <= cap else cap + 1)
                dig.append(d)
                ver.append(1 if tlen <= cap and d == exp else 0)
                sha[c].reset()
            else:
                tsz.append(keep32)
                dig.append(bytes([keep]) * 20)
                ver.append(keep)
            call.add(c, int(states[c]), off, len(piece), final, exp, slot, cap)
            enc_rec[int(states[c])] = E.record(enc[c])
            sha_rec[int(states[c])] = sha[c].record()
        lists = {"new_offsets": noff, "new_lens": nlen, "text_sizes": tsz, "verdicts": ver}
        if route not in HOST:
            lists["digests"] = dig
        _finish(call, lists)
        call.want.update(arena=arena.copy(), rec=list(enc_rec), sha=list(sha_rec))
        sc.calls.append(call)
    for c, ch in enumerate(sc.chains):  # cut independence is asked of the whole chunk's text
        ch["whole"] = E.whole_text(ch["data"], LAYOUTS.index(ch["layout"]))


# ------------------------------------------------------------------------- shot
def _bound(rng, values):
    """A max_* argument: the largest value, or (a third of the time) one that leaves a few chunks over it."""
    top = max(values, default=0)
    if rng.random() < 0.35 and len(values) > 2:
        v = sorted(values)
        return max(int(v[int(rng.integers(len(v) // 2, len(v)))]) - 1, 0)
    return top + (int(rng.integers(0, 100)) if rng.random() < 0.3 else 0)


def _shot_decode(sc, rng):
    n = int(rng.integers(1, 33))
    big = 2
    exp = []
    for c in range(n):
        cls = int(rng.integers(0, 7))
        if cls == 6:
            cls, big = (6, big - 1) if big else (4, big)
        size = _draw_size(rng, cls)
        layout = LAYOUTS[int(rng.integers(0, 2))]
        data = _rand(rng, size)
        clean = text_of(data, layout)
        edges = sorted(int(x) for x in rng.integers(0, len(clean) + 1, 2))
        text, dmg = _damaged(rng, clean, edges)
        w = W.decode(text)
        rel = CAP_RELATIONS[int(rng.integers(0, 3))] if rng.random() < 0.3 else "equal"
        if rel == "shorter" and not w:
            rel = "equal"
        cap = (len(w) if rel == "equal" else int(rng.integers(0, len(w))) if rel == "shorter"
               else len(w) + int(rng.integers(1, 40)))
        e, word = _wrong(rng, hashlib.sha1(data).digest())
        if not (cap == len(w) and w == data):
            word = None  # the verdict is 0 whatever the digest
        exp.append(e)
        tphase, sphase = int(rng.integers(0, 16)), int(rng.integers(0, 16))
        sc.chains.append({"desc": f"chunk {c}: {size} B {layout}, damage {dmg}, {len(text)} characters decode to {len(w)}, "
                                  f"cap {cap} ({rel})", "layout": layout, "size_class": SIZE_CLASSES[cls], "cap_rel": rel,
                          "damage": dmg, "visits": [], "wrong_word": word, "tphases": [tphase], "sphase": sphase, "cap": cap,
                          "slot": sc.slot(cap, sphase, c), "off": sc.place(text, tphase), "text": text, "decoded": w})
    sc.n_states = 0
    max_text_len = _bound(rng, [len(ch["text"]) for ch in sc.chains])
    max_size = _bound(rng, [ch["cap"] for ch in sc.chains])
    # every digests / verdicts null combination
    _decode_calls(sc, exp, max_text_len, max_size, [(d, v) for d in (True, False) for v in (True, False)])


def _decode_calls(sc, exp, max_text_len, max_size, combos):
    """lbf_b64_verify_launch over the scene's chunks (chains with text, off, slot,
    cap, decoded), once per (digests, verdicts) of `combos`."""
    n = len(sc.chains)
    arena = np.full(sc.dst_len + 19, FILL, dtype=np.uint8)
    sc.dst_len = arena.size
    osz, dig, ver = [], [], []
    for c, ch in enumerate(sc.chains):
        cap, w = ch["cap"], ch["decoded"]
        if len(ch["text"]) > max_text_len or cap > max_size:
            osz.append(UINT32_MAX)
            dig.append(EMPTY_SHA)
            ver.append(0)
            ch["desc"] += ", over a bound"
            ch["wrong_word"] = None
            continue
        kept = w[:cap]
        arena[ch["slot"]:ch["slot"] + cap] = np.frombuffer(kept + bytes(cap - len(kept)), dtype=np.uint8)
        osz.append(len(w) if len(w) <= cap else cap + 1)
        dig.append(hashlib.sha1(kept).digest())
        ver.append(1 if len(w) == cap and dig[-1] == exp[c] else 0)
    for digests, verdicts in combos:
        call = Call("verify_b64_launch", fresh=True, max_text_len=max_text_len, max_size=max_size, digests=digests,
                    verdicts=verdicts)
        for c, ch in enumerate(sc.chains):
            call.add(c, 0, ch["off"], len(ch["text"]), True, exp[c], ch["slot"], ch["cap"])
        _finish(call, {"out_sizes": osz, "verdicts": ver if verdicts else [FILL] * n,
                       "digests": dig if digests else [bytes([FILL]) * 20] * n})
        call.want["arena"] = arena
        sc.calls.append(call)


def _shot_encode(sc, rng):
    n = int(rng.integers(1, 33))
    sc.n_states = 0
    sizes = []
    for c in range(n):
        lo, hi = SEED_SIZES[int(rng.integers(0, len(SEED_SIZES) - (1 if c > 4 else 0)))]
        sizes.append(int(rng.integers(lo, hi)))
    max_size = _bound(rng, sizes)
    datas = [_rand(rng, s) for s in sizes]
    offs = [sc.place(d, int(rng.integers(0, 16))) for d in datas]
    exp = [_wrong(rng, hashlib.sha1(d).digest()) for d in datas]
    for c in range(n):
        sc.chains.append({"desc": f"chunk {c}: {sizes[c]} B" + (", over max_size" if sizes[c] > max_size else ""),
                          "visits": [], "wrong_word": exp[c][1] if sizes[c] <= max_size else None, "data": datas[c]})
    _encode_calls(sc, rng, datas, offs, [e for e, _ in exp], max_size, [int(x) for x in rng.permutation(2)])


def _encode_calls(sc, rng, datas, offs, exp, max_size, layouts):
    """lbf_verify_encode_b64_launch over the chunks, once per layout, each into a part of the arena of its own."""
    start = 0
    for layout in layouts:
        sc.dst_len = start
        texts = [E.whole_text(d, layout) for d in datas]
        slots = [sc.slot(len(t), int(rng.integers(0, 16)), c) for c, t in enumerate(texts)]
        call = Call("verify_encode_b64_launch", fresh=True, max_size=max_size, layout=LAYOUTS[layout])
        call.arena_len = sc.dst_len + 19
        arena = np.full(call.arena_len, FILL, dtype=np.uint8)
        loose = np.zeros(call.arena_len, dtype=bool)
        ver = []
        for c, t in enumerate(texts):
            arena[slots[c]:slots[c] + len(t)] = np.frombuffer(t, dtype=np.uint8)
            over = len(datas[c]) > max_size
            if over:  # an incomplete text: every character that is there is right
                loose[slots[c]:slots[c] + len(t)] = True
            ver.append(1 if not over and exp[c] == hashlib.sha1(datas[c]).digest() else 0)
            call.add(c, 0, offs[c], len(datas[c]), True, exp[c], slots[c], len(t))
        _finish(call, {"verdicts": ver, "digests": [hashlib.sha1(d).digest() for d in datas]})
        call.want.update(arena=arena, loose=loose)
        sc.calls.append(call)
        start = sc.dst_len
    sc.dst_len = max(call.arena_len for call in sc.calls)
    for call in sc.calls:  # one arena length for the scene: the part behind a call's own is fill
        grow = sc.dst_len - call.want["arena"].size
        call.want["arena"] = np.concatenate([call.want["arena"], np.full(grow, FILL, dtype=np.uint8)])
        call.want["loose"] = np.concatenate([call.want["loose"], np.zeros(grow, dtype=bool)])


def _shot_scene(sc, rng):
    if rng.random() < 0.6:
        sc.kind = "decode"
        _shot_decode(sc, rng)
    else:
        sc.kind = "encode"
        _shot_encode(sc, rng)


def case(seed: int) -> Scene:
    """The scene of `seed`: deterministic, family seed % 4."""
    family = FAMILIES[seed % 4]
    sc = Scene(seed, family)
    rng = np.random.default_rng([int(seed), 0x91ECE])
    {"hash": _hash_scene, "text": _text_scene, "seed": _seed_scene, "shot": _shot_scene}[family](sc, rng)
    sc.src = np.frombuffer(bytes(sc.src) + bytes([FILL]) * 17, dtype=np.uint8)
    return sc


# ------------------------------------------------- two scenes that are not drawn
BITS, BITS_RIGHT = 160, 32
BITS_ROUTES = ("uniform_launch", "batch_launch", "update_launch", "update_seq_launch", "b64_update_launch",
               "b64_encode_update_launch", "verify_b64_launch", "verify_encode_b64_launch")


def bits_scene(route: str, layout: str = "xmlrpc") -> Scene:
    """Every bit of the expected digest decides the verdict: 192 tiny chains,
    chain k < 160 with bit k of its expected digest wrong (bit k % 8 of byte
    k // 8), the last 32 right, so the verdicts must be 160 zeros and 32 ones.
    One call of `route`, every piece final (two pieces a chain on the seq
    route).  The chunks are 57..96 bytes, where the two text layouts differ;
    the uniform launch has chunks of 61."""
    n = BITS + BITS_RIGHT
    family = {"update_launch": "hash", "update_seq_launch": "hash", "uniform_launch": "hash", "batch_launch": "hash",
              "b64_update_launch": "text", "b64_encode_update_launch": "seed"}.get(route, "shot")
    sc = Scene(f"bits/{route}/{layout}", family)
    sc.kind = "bits"
    lay = LAYOUTS.index(layout)
    datas = [W.chunk_bytes(61 if route == "uniform_launch" else 57 + k % 40, seed=k) for k in range(n)]
    exp = []
    for k, d in enumerate(datas):
        e = bytearray(hashlib.sha1(d).digest())
        if k < BITS:
            e[k // 8] ^= 1 << (k % 8)
        exp.append(bytes(e))
        sc.chains.append({"desc": f"chain {k}: {len(d)} B {layout}, " + (f"bit {k} wrong" if k < BITS else "right"),
                          "visits": [], "wrong_word": k // 32 if k < BITS else None, "data": d, "layout": layout})
    ver = [0] * BITS + [1] * BITS_RIGHT
    dig = [hashlib.sha1(d).digest() for d in datas]
    if family == "hash":
        sc.n_states = 0 if route in ("uniform_launch", "batch_launch") else n
        if route == "uniform_launch":
            base = sc.place(b"".join(datas), 0)
            offs = [base + 61 * k for k in range(n)]
            call = Call(route, chunk_size=61)
        else:
            offs = [sc.place(d, k % 16) for k, d in enumerate(datas)]
            call = Call(route)
        want_dig, want_ver = [], []
        for k, d in enumerate(datas):
            if route == "update_seq_launch":  # a piece that is not final in front
                call.add(k, k, offs[k], 30, False, bytes(20))
                call.add(k, k, offs[k] + 30, len(d) - 30, True, exp[k])
                want_dig += [bytes([FILL]) * 20, dig[k]]
                want_ver += [FILL, ver[k]]
            else:
                call.add(k, k, offs[k], len(d), True, exp[k])
                want_dig.append(dig[k])
                want_ver.append(ver[k])
        _finish(call, {"verdicts": want_ver, "digests": want_dig})
        if sc.n_states:
            call.want["sha"] = [SHA_INIT] * n
        sc.calls.append(call)
    elif family == "text":
        sc.n_states = n
        call = Call(route)
        texts = [text_of(d, layout) for d in datas]
        for k, (d, t) in enumerate(zip(datas, texts)):
            sc.chains[k].update(cap=len(d), slot=sc.slot(len(d), k % 16, k))
            call.add(k, k, sc.place(t, (5 * k) % 16), len(t), True, exp[k], sc.chains[k]["slot"], len(d))
        arena = np.full(sc.dst_len + 19, FILL, dtype=np.uint8)
        sc.dst_len = arena.size
        for k, d in enumerate(datas):
            arena[sc.chains[k]["slot"]:sc.chains[k]["slot"] + len(d)] = np.frombuffer(d, dtype=np.uint8)
        _finish(call, {"out_sizes": [len(d) for d in datas], "verdicts": ver, "digests": dig})
        call.want.update(arena=arena, rec=[M.b64_record(M.init())] * n, sha=[SHA_INIT] * n)
        sc.calls.append(call)
    elif family == "seed":
        sc.n_states, sc.enc_layouts = n, [lay] * n
        call = Call(route)
        texts = [E.whole_text(d, lay) for d in datas]
        for k, (d, t) in enumerate(zip(datas, texts)):
            sc.chains[k].update(cap=len(t), slot=sc.slot(len(t), k % 16, k))
            call.add(k, k, sc.place(d, (5 * k) % 16), len(d), True, exp[k], sc.chains[k]["slot"], len(t))
        arena = np.full(sc.dst_len + 19, FILL, dtype=np.uint8)
        sc.dst_len = arena.size
        for k, t in enumerate(texts):
            arena[sc.chains[k]["slot"]:sc.chains[k]["slot"] + len(t)] = np.frombuffer(t, dtype=np.uint8)
        _finish(call, {"new_offsets": [ch["slot"] for ch in sc.chains], "new_lens": [len(t) for t in texts],
                       "text_sizes": [len(t) for t in texts], "verdicts": ver, "digests": dig})
        call.want.update(arena=arena, rec=[E.record(E.init(lay))] * n, sha=[SHA_INIT] * n)
        sc.calls.append(call)
    elif route == "verify_b64_launch":
        for k, d in enumerate(datas):
            t = text_of(d, layout)
            sc.chains[k].update(cap=len(d), slot=sc.slot(len(d), k % 16, k), off=sc.place(t, (5 * k) % 16), text=t, decoded=d)
        _decode_calls(sc, exp, max(len(ch["text"]) for ch in sc.chains), max(len(d) for d in datas), [(True, True)])
    else:
        offs = [sc.place(d, (5 * k) % 16) for k, d in enumerate(datas)]
        _encode_calls(sc, np.random.default_rng(160), datas, offs, exp, max(len(d) for d in datas), [lay])
    if family == "shot":
        assert sc.calls[0].want["verdicts"].tolist() == ver
    sc.src = np.frombuffer(bytes(sc.src) + bytes([FILL]) * 17, dtype=np.uint8)
    return sc


SELECTION_CHUNKS = 16390   # past 16,384 chunks the automatic selection takes pc4x2, up to 32,768


def selection_scene(route: str) -> Scene:
    """The 16 K-32 K kernel selection behind the wire kernels: 16,390 chunks of
    3..55 bytes in mixed layouts, every 97th with a wrong expected digest, every
    101st text damaged (the kinds in turn), through lbf_b64_verify_launch (one
    call, layouts and damage mixed) or lbf_verify_encode_b64_launch (a call per
    layout)."""
    n = SELECTION_CHUNKS
    rng = np.random.default_rng(16390)
    sc = Scene(f"selection/{route}", "shot")
    sc.kind = "selection"
    sizes = rng.integers(3, 56, n)
    stream = _rand(rng, int(sizes.sum()))
    at = np.concatenate([[0], np.cumsum(sizes)])
    datas = [stream[at[k]:at[k + 1]] for k in range(n)]
    exp = []
    for k, d in enumerate(datas):
        e = bytearray(hashlib.sha1(d).digest())
        if k % 97 == 5:
            e[(k // 97) % 20] ^= 1 << (k % 8)
        exp.append(bytes(e))
    if route == "verify_encode_b64_launch":
        for k, d in enumerate(datas):
            sc.chains.append({"desc": f"chunk {k}: {len(d)} B", "visits": [], "wrong_word": None, "data": d})
        offs = [sc.place(d, int(p)) for d, p in zip(datas, rng.integers(0, 16, n))]
        _encode_calls(sc, rng, datas, offs, exp, 55, [0, 1])
    else:
        for k, d in enumerate(datas):
            layout = LAYOUTS[int(rng.integers(0, 2))]
            t = text_of(d, layout)
            dmg = None
            if k % 101 == 7:
                kind = W.KINDS[(k // 101) % len(W.KINDS)]
                dmg = (kind, int(rng.integers(0, len(t))))
                t = W.damage(t, *dmg)
            sc.chains.append({"desc": f"chunk {k}: {len(d)} B {layout}, damage {dmg}", "visits": [], "wrong_word": None,
                              "layout": layout, "damage": dmg, "cap": len(d), "text": t, "decoded": W.decode(t),
                              "slot": sc.slot(len(d), int(rng.integers(0, 16)), k),
                              "off": sc.place(t, int(rng.integers(0, 16)))})
        _decode_calls(sc, exp, max(len(ch["text"]) for ch in sc.chains), 55, [(True, True)])
    sc.src = np.frombuffer(bytes(sc.src) + bytes([FILL]) * 17, dtype=np.uint8)
    return sc


# ---------------------------------------------------------------------- checker
def check(sc: Scene, k: int, got: dict) -> None:
    """Hold `got`, what call k gave, against its expectation.  got: "arena"
    (uint8, the whole output arena), the PER_PIECE arrays in caller order, "rec"
    (per state, the decoder's or encoder's record as a tuple of its fields),
    "sha" (per state: (h as a tuple, total, buffered, the 64 block bytes)); only
    the keys the expectation holds are read, and all of those must be there."""
    call, want = sc.calls[k], sc.calls[k].want

    def fail(place, chain=None):
        raise Mismatch(sc.describe(k, place, chain))

    if "arena" in want:
        g, w = np.asarray(got["arena"]), want["arena"]
        if g.shape != w.shape:
            fail(f"the arena is {g.shape} bytes, not {w.shape}")
        bad = g != w
        if "loose" in want:
            bad &= ~(want["loose"] & (g == FILL))
        if bad.any():
            pos = int(np.flatnonzero(bad)[0])
            chain = next((c for s, n, c in sc.slots if s <= pos < s + n), None)
            fail(f"arena byte {pos} is 0x{int(g[pos]):02x}, not 0x{int(w[pos]):02x} ({int(bad.sum())} bytes differ): "
                 f"{sc.where(pos)}", chain)
    for key in PER_PIECE:
        if key not in want:
            continue
        g, w = np.asarray(got[key]), want[key]
        if g.shape != w.shape:
            fail(f"{key} has shape {g.shape}, not {w.shape}")
        bad = (g != w).reshape(w.shape[0], -1).any(axis=1)
        if bad.any():
            i = int(np.flatnonzero(bad)[0])
            show = (lambda a: bytes(a).hex()) if key == "digests" else int
            fail(f"{key}[{i}] is {show(g[i])}, not {show(w[i])} (piece {i} of {call.n}, final {call.final[i]}, "
                 f"{call.src_len[i]} bytes at {call.src_off[i]}; {int(bad.sum())} entries differ)", call.chain[i])
    chain_of = {}
    for c, s in zip(call.chain, call.state_of):
        chain_of.setdefault(s, c)
    if "rec" in want:
        names = ENC_FIELDS if sc.family == "seed" else B64_FIELDS
        if len(got["rec"]) != len(want["rec"]):
            fail(f"{len(got['rec'])} records, not {len(want['rec'])}")
        for s, (g, w) in enumerate(zip(got["rec"], want["rec"])):
            for name, a, b in zip(names, g, w):
                if int(a) != int(b):
                    fail(f"record {s}'s {name} is {int(a)}, not {int(b)} (record {tuple(int(x) for x in g)}, not {w})",
                         chain_of.get(s))
    if "sha" in want:
        if len(got["sha"]) != len(want["sha"]):
            fail(f"{len(got['sha'])} SHA-1 records, not {len(want['sha'])}")
        for s, (g, w) in enumerate(zip(got["sha"], want["sha"])):
            gh, gtotal, gbuf, gblock = g
            wh, wtotal, wbuf, wblock = w
            if int(gtotal) != wtotal:
                fail(f"SHA-1 record {s}'s total is {int(gtotal)}, not {wtotal}", chain_of.get(s))
            if int(gbuf) != wbuf:
                fail(f"SHA-1 record {s}'s buffered is {int(gbuf)}, not {wbuf}", chain_of.get(s))
            if bytes(gblock)[:wbuf] != wblock:
                fail(f"SHA-1 record {s}'s block is {bytes(gblock)[:wbuf].hex()}, not {wblock.hex()}", chain_of.get(s))
            if wh is not None and tuple(int(x) for x in gh) != wh:
                fail(f"SHA-1 record {s}'s h is {[hex(int(x)) for x in gh]}, not {[hex(x) for x in wh]}", chain_of.get(s))


def as_result(sc: Scene, k: int) -> dict:
    """Call k's own expectation in the shape of a result (copies; an h that is not followed as zeros)."""
    want = sc.calls[k].want
    got = {key: want[key].copy() for key in ("arena",) + PER_PIECE if key in want}
    if "rec" in want:
        got["rec"] = [tuple(r) for r in want["rec"]]
    if "sha" in want:
        got["sha"] = [((0,) * 5 if h is None else h, total, buf, block + bytes(64 - len(block)))
                      for h, total, buf, block in want["sha"]]
    return got

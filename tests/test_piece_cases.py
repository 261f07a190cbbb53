"""The random scenes of tests/piece_cases.py and their checker, on the CPU: what
the fixed slice reaches (the ledger), that a scene's piece-by-piece expectation
is the whole chunk's answer whatever the cuts and routes, and that the checker
catches every kind of wrong result and says where.  tests/test_gpu_piece_fuzz.py
runs the same slice on the GPU.
"""
import base64
import collections
import hashlib
import itertools
import os

import numpy as np
import pytest

from tests import piece_cases as P
from tests import sha1_model
from tests import wire_encode_model as E
from tests import wire_layouts as W


@pytest.fixture(scope="module")
def scenes():
    """Every scene of the slice, built once: {family: [scene]}.  The tests only read them."""
    return {fam: [P.case(s) for s in seeds] for fam, seeds in P.SLICE.items()}


def test_a_seed_is_a_scene_and_names_its_family():
    for fam, seeds in P.SLICE.items():
        assert len(set(seeds)) == len(seeds) and all(P.FAMILIES[s % 4] == fam for s in seeds)
    for seed in (P.SLICE["hash"][0], P.SLICE["text"][3], P.SLICE["seed"][1], P.SLICE["shot"][2]):
        a, b = P.case(seed), P.case(seed)
        assert a.src.tobytes() == b.src.tobytes() and len(a.calls) == len(b.calls) > 0
        for x, y in zip(a.calls, b.calls):
            assert (x.route, x.switches, x.src_off, x.state_of, x.expected) == (y.route, y.switches, y.src_off, y.state_of,
                                                                               y.expected)
            assert all(np.array_equal(x.want[k], y.want[k]) for k in x.want if isinstance(x.want[k], np.ndarray))


def test_only_inputs_the_contract_allows(scenes):
    """Pieces inside the input arena, slots inside the output arena and apart
    from one another, one piece per chain in the one-piece calls, a final piece
    last among its chain's pieces of the call, states in range and one per chain."""
    for sc in itertools.chain.from_iterable(scenes.values()):
        slots = sorted(sc.slots)
        for (a, n, _), (b, _, _) in zip(slots, slots[1:]):
            assert a + n <= b, sc.seed
        assert all(a + n <= sc.dst_len for a, n, _ in slots), sc.seed
        for k, call in enumerate(sc.calls):
            assert call.n > 0 and call.route in P.ROUTES[sc.family]
            assert all(0 <= o and o + n <= sc.src.size for o, n in zip(call.src_off, call.src_len)), (sc.seed, k)
            if sc.family == "shot":
                continue
            assert all(0 <= s < sc.n_states for s in call.state_of)
            assert len({(c, s) for c, s in zip(call.chain, call.state_of)}) == len(set(call.state_of)) == len(set(call.chain))
            if call.route not in P.SEQ:
                assert len(set(call.state_of)) == call.n, (sc.seed, k)
            last = {s: i for i, s in enumerate(call.state_of)}
            assert all(not f or last[s] == i for i, (s, f) in enumerate(zip(call.state_of, call.final))), (sc.seed, k)
            if sc.family != "hash":
                assert all((o, n, c) in sc.slots for o, n, c in zip(call.dst_off, call.cap, call.chain))


def _classes(scenes):
    """The ledger's counts over the slice."""
    led = collections.defaultdict(collections.Counter)
    for fam in ("hash", "text", "seed"):
        for sc in scenes[fam]:
            for call in sc.calls:
                led["live"][_live_class(len(set(call.state_of)))] += 1
                if call.switches is not None:
                    led["switches"][call.switches] += 1
            for ch in sc.chains:
                for (_, r0, s0, _), (_, r1, s1, pending) in zip(ch["visits"], ch["visits"][1:]):
                    led[fam + " pairs"][(r0, r1)] += 1
                    if fam == "text":
                        if s0 != s1:
                            led["switch change at"][pending] += 1
                        if r0 != r1:
                            led["text handed over at"][(ch["layout"], pending)] += 1
                    elif fam == "seed" and r0 != r1:
                        led["seed handed over at"][(ch["layout"], pending)] += 1
                    elif fam == "hash" and r0 != r1:
                        led["hash handed over at"]["0" if pending == 0 else "1..55" if pending < 56 else "56..63"] += 1
                if ch["wrong_word"] is not None:
                    led[fam + " wrong word"][ch["wrong_word"]] += 1
                    led["wrong word"][ch["wrong_word"]] += 1
    for sc in scenes["text"]:
        for ch in sc.chains:
            if ch["damage"] and ch["fed"] > ch["damage"][2]:
                led["damage"][(ch["damage"][0], ch["damage"][1], ch["layout"])] += 1
            if ch["fed"]:
                led["size class"][ch["size_class"]] += 1
                led["cap"][ch["cap_rel"]] += 1
                led["slot phase"][ch["sphase"]] += 1
            for ph in ch["tphases"]:
                led["text phase"][ph] += 1
    for fam in ("hash", "seed"):
        for sc in scenes[fam]:
            for ch in sc.chains:
                for ph in ch["sphases"]:
                    led["source phase"][ph] += 1
                if fam == "seed" and ch["visits"]:
                    led["text cap"][ch["cap_rel"]] += 1
                    led["text slot phase"][ch["sphase"]] += 1
    for sc in scenes["shot"]:
        led["shot"][sc.kind] += 1
        for call in sc.calls:
            o = call.opts
            if sc.kind == "decode":
                led["shot nulls"][(o["digests"], o["verdicts"])] += 1
                led["shot bounds"][("text below" if o["max_text_len"] < max(call.src_len) else "text",
                                    "size below" if o["max_size"] < max(call.cap) else "size")] += 1
            else:
                led["shot layouts"][(o["layout"], "below" if o["max_size"] < max(call.src_len) else "max")] += 1
        for ch in sc.chains:
            if ch["wrong_word"] is not None:
                led["shot wrong word"][ch["wrong_word"]] += 1
            if sc.kind == "decode" and ch["damage"]:
                led["shot damage"][ch["damage"][0]] += 1
    return led


def _live_class(n):
    return "1" if n == 1 else "2..63" if n < 64 else "64" if n == 64 else "65..128" if n <= 128 else "129+"


def test_the_ledger_of_the_slice(scenes):
    """What the fixed slice reaches; a class the slice misses fails here, not silently on the GPU."""
    led = _classes(scenes)

    def need(name, keys, at_least=1):
        short = {k: led[name][k] for k in keys if led[name][k] < at_least}
        assert not short, f"{name}: fewer than {at_least} of {short}; have {dict(led[name])}"

    for fam in ("hash", "text", "seed"):
        pairs = list(itertools.product(P.ROUTES[fam], repeat=2))
        assert len(pairs) == (4 if fam == "seed" else 16)
        need(fam + " pairs", pairs, 3)
    need("switches", list(itertools.product((0, 1), repeat=3)), 3)
    need("switch change at", [1, 2, 3])
    need("text handed over at", list(itertools.product(P.LAYOUTS, (0, 1, 2, 3))))
    need("seed handed over at", list(itertools.product(P.LAYOUTS, (0, 1, 2))))
    need("hash handed over at", ["0", "1..55", "56..63"])
    need("damage", list(itertools.product(W.KINDS, ("first", "middle", "last"), P.LAYOUTS)))
    need("size class", P.SIZE_CLASSES)
    need("cap", P.CAP_RELATIONS)
    need("text cap", P.TEXT_CAPS)
    for name in ("text phase", "slot phase", "source phase", "text slot phase"):
        need(name, range(16))
    need("live", ["1", "2..63", "64", "65..128", "129+"])
    for name in ("wrong word", "hash wrong word", "text wrong word", "seed wrong word", "shot wrong word"):
        need(name, range(5))
    need("shot", ["decode", "encode"], 3)
    need("shot nulls", list(itertools.product((True, False), repeat=2)), 3)
    need("shot bounds", [("text below", "size"), ("text", "size below"), ("text", "size")])
    need("shot layouts", list(itertools.product(P.LAYOUTS, ("below", "max"))))
    need("shot damage", W.KINDS)


def test_the_model_checked_bytes_stay_within_the_budget(scenes):
    """Per scene at most H_BUDGET bytes go through tests/sha1_model.py, so GROUP scenes stay within 512 KiB;
    and the budget is not idle: records with a followed h that is not the initial one exist in every family."""
    assert P.GROUP * P.H_BUDGET <= 512 << 10
    for fam in ("hash", "text", "seed"):
        followed = 0
        for sc in scenes[fam]:
            assert 0 <= sc.h_left <= P.H_BUDGET
            for call in sc.calls:
                followed += sum(1 for h, total, _, _ in call.want["sha"] if h is not None and total >= 64)
        assert followed > 20, (fam, followed)


def test_cut_independence(scenes):
    """Piece by piece equals the whole chunk, whatever the cuts and the routes:
    a finished chain's slot holds W.decode of its whole text (up to the cap), its
    size and digest are the whole text's, its verdict the whole chunk's; a
    finished seeder chain's slot holds E.whole_text; a finished hash chain's
    digest is hashlib's of all its pieces."""
    finished = collections.Counter()
    for sc in scenes["text"]:
        last = sc.calls[-1].want["arena"]
        for c, ch in enumerate(sc.chains):
            w = W.decode(ch["text"])
            assert w == ch["decoded"] and b"".join(ch["pieces"]) == ch["text"]
            ends = [(k, i) for k, call in enumerate(sc.calls) for i in range(call.n) if call.chain[i] == c and call.final[i]]
            if not ends:
                continue
            (k, i), = ends
            want, cap = sc.calls[k].want, ch["cap"]
            kept = w[:cap]
            assert last[ch["slot"]:ch["slot"] + len(kept)].tobytes() == kept, (sc.seed, c)
            assert (last[ch["slot"] + len(kept):ch["slot"] + cap] == P.FILL).all(), (sc.seed, c)
            assert int(want["out_sizes"][i]) == (len(w) if len(w) <= cap else cap + 1), (sc.seed, c)
            ok = len(w) == cap and hashlib.sha1(w).digest() == sc.calls[k].expected[i]
            assert int(want["verdicts"][i]) == int(ok), (sc.seed, c)
            if "digests" in want:
                assert want["digests"][i].tobytes() == hashlib.sha1(kept).digest(), (sc.seed, c)
            finished["text"] += 1
    for sc in scenes["seed"]:
        last = sc.calls[-1].want["arena"]
        for c, ch in enumerate(sc.chains):
            whole = E.whole_text(ch["data"], P.LAYOUTS.index(ch["layout"]))
            assert whole == (W.xmlrpc_text(ch["data"]) if ch["layout"] == "xmlrpc" else base64.b64encode(ch["data"]))
            ends = [(k, i) for k, call in enumerate(sc.calls) for i in range(call.n) if call.chain[i] == c and call.final[i]]
            if not ends:
                continue
            (k, i), = ends
            want, cap = sc.calls[k].want, ch["cap"]
            assert last[ch["slot"]:ch["slot"] + cap].tobytes() == whole[:cap], (sc.seed, c)
            assert int(want["text_sizes"][i]) == (len(whole) if len(whole) <= cap else cap + 1)
            ok = len(whole) <= cap and hashlib.sha1(ch["data"]).digest() == sc.calls[k].expected[i]
            assert int(want["verdicts"][i]) == int(ok), (sc.seed, c)
            finished["seed"] += 1
    for sc in scenes["hash"]:
        pieces = collections.defaultdict(bytes)
        for k, call in enumerate(sc.calls):
            for i in range(call.n):
                c = call.chain[i]
                pieces[c] += sc.src[call.src_off[i]:call.src_off[i] + call.src_len[i]].tobytes()
                if call.final[i]:
                    d = hashlib.sha1(pieces[c]).digest()
                    if "digests" in call.want:
                        assert call.want["digests"][i].tobytes() == d, (sc.seed, c)
                    if "verdicts" in call.want:
                        assert int(call.want["verdicts"][i]) == int(d == call.expected[i]), (sc.seed, c)
                    finished["hash"] += 1
            # an unfinished chain's record is the model's over all its pieces so far, where h is followed
            for c, s in set(zip(call.chain, call.state_of)):
                h, total, buffered, block = call.want["sha"][s]
                if total and h is not None and total <= 4096:
                    mh, mtotal, mblock = sha1_model.update(sha1_model.init(), pieces[c])
                    assert (h, total, buffered, block) == (tuple(mh), mtotal, len(mblock), mblock), (sc.seed, c)
    for sc in scenes["shot"]:
        for call in sc.calls:
            for i, c in enumerate(call.chain):
                if sc.kind == "encode":
                    data = sc.chains[c]["data"]
                    whole = W.xmlrpc_text(data) if call.opts["layout"] == "xmlrpc" else base64.b64encode(data)
                    assert call.want["arena"][call.dst_off[i]:call.dst_off[i] + call.cap[i]].tobytes() == whole
                    finished["shot"] += 1
    assert min(finished[f] for f in P.FAMILIES) >= 50, finished


# --------------------------------------------------------- the checker catches mutants
def _must_fail(sc, k, got, *words):
    with pytest.raises(P.Mismatch) as e:
        P.check(sc, k, got)
    msg = str(e.value)
    for w in (f"seed {sc.seed} ", f"call {k} ", sc.calls[k].route,
              f"python tools/fuzz_pieces.py --seed {sc.seed} --cases 1") + words:
        assert w in msg, (w, msg)


def _first_call(scenes, fam, pred):
    for sc in scenes[fam]:
        for k, call in enumerate(sc.calls):
            if pred(sc, call):
                return sc, k
    raise AssertionError(f"no {fam} call of the slice fits")


def test_the_expectation_itself_passes(scenes):
    for sc in itertools.chain.from_iterable(scenes.values()):
        for k in range(len(sc.calls)):
            P.check(sc, k, P.as_result(sc, k))


@pytest.mark.parametrize("fam", ["text", "seed", "shot"])
def test_checker_catches_arena_bytes(scenes, fam):
    sc, k = _first_call(scenes, fam, lambda sc, call: any(call.cap) and (call.want["arena"] != P.FILL).any())
    call = sc.calls[k]
    inside = int(np.flatnonzero(call.want["arena"] != P.FILL)[0])
    got = P.as_result(sc, k)
    got["arena"][inside] ^= 0x01
    chain = next(c for s, n, c in sc.slots if s <= inside < s + n)
    _must_fail(sc, k, got, f"arena byte {inside} ", f"slot of chain {chain}", sc.chains[chain]["desc"])
    taken = np.zeros(sc.dst_len, dtype=bool)
    for s, n, _ in sc.slots:
        taken[s:s + n] = True
    outside = int(np.flatnonzero(~taken)[-1])
    got = P.as_result(sc, k)
    got["arena"][outside] = 0
    _must_fail(sc, k, got, f"arena byte {outside} ", "outside every slot")
    # a slot byte that had to keep its fill
    if fam == "text":
        kept = np.flatnonzero(taken & (call.want["arena"] == P.FILL))
        assert kept.size
        got = P.as_result(sc, k)
        got["arena"][int(kept[0])] = 0
        _must_fail(sc, k, got, f"arena byte {int(kept[0])} ")


def test_a_loose_slot_takes_fill_or_the_right_character_only(scenes):
    """A chunk over max_size has an incomplete text: a character left at its fill passes, a wrong one does not."""
    sc, k = _first_call(scenes, "shot", lambda sc, call: "loose" in call.want and call.want["loose"].any())
    at = int(np.flatnonzero(sc.calls[k].want["loose"])[0])
    got = P.as_result(sc, k)
    got["arena"][at] = P.FILL
    P.check(sc, k, got)
    got["arena"][at] = ord("*")
    _must_fail(sc, k, got, f"arena byte {at} ")


@pytest.mark.parametrize("fam,key", [("text", "out_sizes"), ("shot", "out_sizes"), ("seed", "text_sizes"),
                                     ("seed", "new_lens"), ("seed", "new_offsets"), ("hash", "verdicts"),
                                     ("text", "verdicts"), ("seed", "verdicts"), ("shot", "verdicts")])
def test_checker_catches_a_table_entry(scenes, fam, key):
    """One entry of a per-piece result, at a final piece and at one that is not (which keeps its fill)."""
    for final in (1, 0):
        if final == 0 and (fam == "shot" or key in ("new_lens", "new_offsets")):
            continue
        sc, k = _first_call(scenes, fam, lambda sc, call: key in call.want and final in call.final
                            and call.opts.get("verdicts", True))
        i = sc.calls[k].final.index(final)
        got = P.as_result(sc, k)
        got[key][i] ^= 1
        _must_fail(sc, k, got, f"{key}[{i}] ", sc.chains[sc.calls[k].chain[i]]["desc"])


@pytest.mark.parametrize("fam", P.FAMILIES)
def test_checker_catches_every_digest_bit(scenes, fam):
    sc, k = _first_call(scenes, fam, lambda sc, call: "digests" in call.want and 1 in call.final
                        and call.opts.get("digests", True))
    i = sc.calls[k].final.index(1)
    for bit in range(160):
        got = P.as_result(sc, k)
        got["digests"][i, bit // 8] ^= 1 << (bit % 8)
        _must_fail(sc, k, got, f"digests[{i}] ")


@pytest.mark.parametrize("fam,names", [("text", P.B64_FIELDS), ("seed", P.ENC_FIELDS)])
def test_checker_catches_every_record_field(scenes, fam, names):
    """Each field of the decoder's and the encoder's record, on a record the call wrote and on one it left alone."""
    sc, k = _first_call(scenes, fam, lambda sc, call: len(set(call.state_of)) < sc.n_states and 0 in call.final)
    call = sc.calls[k]
    touched = call.state_of[call.final.index(0)]
    idle = next(s for s in range(sc.n_states) if s not in call.state_of)
    for s in (touched, idle):
        for j, name in enumerate(names):
            got = P.as_result(sc, k)
            r = list(got["rec"][s])
            r[j] += 1
            got["rec"][s] = tuple(r)
            _must_fail(sc, k, got, f"record {s}'s {name} ")


@pytest.mark.parametrize("fam", ["hash", "text", "seed"])
def test_checker_catches_every_sha_record_field(scenes, fam):
    def fits(sc, call):
        return any(h is not None and total >= 64 and buffered for h, total, buffered, _ in call.want["sha"])
    sc, k = _first_call(scenes, fam, fits)
    want = sc.calls[k].want["sha"]
    s = next(s for s, (h, total, buffered, _) in enumerate(want) if h is not None and total >= 64 and buffered)
    buffered = want[s][2]
    for word in range(5):
        got = P.as_result(sc, k)
        h = list(got["sha"][s][0])
        h[word] ^= 1 << (7 * word)
        got["sha"][s] = (tuple(h),) + got["sha"][s][1:]
        _must_fail(sc, k, got, f"SHA-1 record {s}'s h ")
    for j, name in ((1, "total"), (2, "buffered")):
        got = P.as_result(sc, k)
        r = list(got["sha"][s])
        r[j] += 1
        got["sha"][s] = tuple(r)
        _must_fail(sc, k, got, f"SHA-1 record {s}'s {name} ")
    for at in (0, buffered - 1):
        got = P.as_result(sc, k)
        block = bytearray(got["sha"][s][3])
        block[at] ^= 0x80
        got["sha"][s] = got["sha"][s][:3] + (bytes(block),)
        _must_fail(sc, k, got, f"SHA-1 record {s}'s block ")
    # the bytes past `buffered` are not the record's: whatever lies there passes
    got = P.as_result(sc, k)
    block = bytearray(got["sha"][s][3])
    block[buffered] ^= 0xFF
    got["sha"][s] = got["sha"][s][:3] + (bytes(block),)
    P.check(sc, k, got)


def test_checker_wants_every_key_and_shape(scenes):
    sc, k = _first_call(scenes, "text", lambda sc, call: True)
    got = P.as_result(sc, k)
    del got["verdicts"]
    with pytest.raises(KeyError):
        P.check(sc, k, got)
    got = P.as_result(sc, k)
    got["out_sizes"] = got["out_sizes"][:-1]
    _must_fail(sc, k, got, "out_sizes has shape")
    got = P.as_result(sc, k)
    got["rec"] = got["rec"][:-1]
    _must_fail(sc, k, got, "records, not")


# ------------------------------------------------ the old drivers' cases in the suite
FUZZ_GPU_SEED, FUZZ_GPU_CASES = 111, 24   # tests/test_gpu_fuzz_drivers.py starts tools/fuzz_gpu.py with these


def test_fuzz_gpu_seed_reaches_every_variant_in_every_mode():
    """tools/fuzz_gpu.py's case k of --seed S has the seed S * 1,000,003 + k; its
    variant and its mode are its first two draws.  Replayed here without a GPU:
    the run the suite starts meets all 15 (variant, mode) pairs."""
    variants = [1, 7, 10, 11, 12]  # tools/fuzz_gpu.py VARIANTS, the shipped ones
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools", "fuzz_gpu.py")) as f:
        src = f.read()
    assert "else [1, 7, 10, 11, 12]" in src and "seed = a.seed * 1_000_003 + k" in src
    assert src.index("v = int(rng.choice(VARIANTS))") < src.index("mode = int(rng.integers(0, 3))") < src.index("if mode == 2:")
    seen = set()
    for k in range(FUZZ_GPU_CASES):
        rng = np.random.default_rng(FUZZ_GPU_SEED * 1_000_003 + k)
        v = int(rng.choice(variants))
        seen.add((v, int(rng.integers(0, 3))))
    assert seen == set(itertools.product(variants, range(3)))


# ------------------------------------------------------ the two scenes that are not drawn
@pytest.mark.parametrize("route", P.BITS_ROUTES)
def test_bits_scene_flips_every_bit_once(route):
    """Chain k < 160 differs from its chunk's digest in bit k alone, the last 32
    not at all, on every route and in both layouts; the expectation is its own result."""
    for layout in P.LAYOUTS:
        sc = P.bits_scene(route, layout)
        call, = sc.calls
        finals = [i for i in range(call.n) if call.final[i]]
        assert len(finals) == P.BITS + P.BITS_RIGHT == 192 and [call.chain[i] for i in finals] == list(range(192))
        for k, i in enumerate(finals):
            data = sc.src[call.src_off[i] + call.src_len[i] - len(sc.chains[k]["data"]):call.src_off[i] + call.src_len[i]]
            if route.startswith(("verify_b64", "b64_update")):
                data = W.decode(sc.src[call.src_off[i]:call.src_off[i] + call.src_len[i]].tobytes())
            diff = int.from_bytes(hashlib.sha1(bytes(data)).digest(), "little") ^ int.from_bytes(call.expected[i], "little")
            assert diff == ((1 << k) if k < P.BITS else 0), (route, layout, k)
        assert call.want["verdicts"][finals].tolist() == [0] * P.BITS + [1] * P.BITS_RIGHT
        assert {sc.chains[k]["wrong_word"] for k in range(P.BITS)} == set(range(5))
        P.check(sc, 0, P.as_result(sc, 0))
        got = P.as_result(sc, 0)
        got["verdicts"][finals[77]] = 1
        with pytest.raises(P.Mismatch, match="bit 77 wrong"):
            P.check(sc, 0, got)


@pytest.mark.parametrize("route", P.ROUTES["shot"])
def test_selection_scene(route):
    """16,390 chunks of 3..55 bytes, both layouts, a few wrong digests and a few damaged texts."""
    sc = P.selection_scene(route)
    assert len(sc.chains) == P.SELECTION_CHUNKS == 16390 and 16384 < 16390 <= 32768
    sizes = [len(ch["data"]) if "data" in ch else ch["cap"] for ch in sc.chains]
    assert min(sizes) == 3 and max(sizes) == 55
    for k, call in enumerate(sc.calls):
        assert call.n == 16390 and call.route == route
        ver = call.want["verdicts"]
        assert 100 < int((ver == 0).sum()) < 600
        P.check(sc, k, P.as_result(sc, k))
    if route == "verify_b64_launch":
        assert len(sc.calls) == 1
        assert {ch["layout"] for ch in sc.chains} == set(P.LAYOUTS)
        assert {ch["damage"][0] for ch in sc.chains if ch["damage"]} == set(W.KINDS)
        # the layouts differ only at 54 and 55 bytes: both are there in both
        assert {(ch["layout"], ch["cap"]) for ch in sc.chains if ch["cap"] >= 54} == set(itertools.product(P.LAYOUTS, (54, 55)))
    else:
        assert [call.opts["layout"] for call in sc.calls] == ["xmlrpc", "flat"]

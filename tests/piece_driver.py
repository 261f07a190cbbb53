"""Runs a tests/piece_cases.py scene on the GPU, call by call, and holds every
call against the scene's expectation -- TEST INFRASTRUCTURE for
tests/test_gpu_piece_fuzz.py and tools/fuzz_pieces.py.

Between two calls the records live as bytes and nowhere else: a call gets them
from `tobytes()` of what the call before it left, as a receiver that stores its
16-byte and 96-byte records would, whichever route wrote them.  The output arena
is carried from call to call in the same way (a `fresh` call starts from 0xEE).
Every table and result array of a launch route is a device allocation of its
own, results pre-filled with 0xEE.  The (lines, flat, fused) switches of a call
are set in front of it and put back behind it, whatever happens.
"""
import numpy as np

from bitflood_amd import (B64_ENC_STATE_DTYPE, B64_STATE_DTYPE, STATE_DTYPE, DeviceBuffer, new_b64_enc_states,
                          new_b64_states, new_states)
from bitflood_amd import hashing as H
from tests import piece_cases as P

FILL = P.FILL


class _Device:
    """Device copies of host arrays, freed together."""

    def __init__(self):
        self.bufs = []

    def put(self, a: np.ndarray) -> DeviceBuffer:
        a = np.ascontiguousarray(a)
        b = DeviceBuffer(max(a.nbytes, 16))
        self.bufs.append(b)
        if a.nbytes:
            b.upload(a)
        return b

    def filled(self, nbytes: int) -> DeviceBuffer:
        return self.put(np.full(max(nbytes, 16), FILL, dtype=np.uint8))

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for b in self.bufs:
            b.free()


def _sha_tuples(states: np.ndarray):
    return [(tuple(int(x) for x in s["h"]), int(s["total"]), int(s["buffered"]), s["block"].tobytes()) for s in states]


def _rec_tuples(states: np.ndarray):
    return [tuple(int(s[name]) for name in states.dtype.names) for s in states]


class Runner:
    def __init__(self, hasher, scene):
        self.h, self.sc = hasher, scene
        n = scene.n_states
        self.sha = new_states(n).tobytes()
        self.rec, self.rec_dtype = b"", None
        if scene.family == "text":
            self.rec, self.rec_dtype = new_b64_states(n).tobytes(), B64_STATE_DTYPE
        elif scene.family == "seed":
            both = [new_b64_enc_states(n, layout) for layout in P.LAYOUTS]
            mine = np.array([both[lay][s] for s, lay in enumerate(scene.enc_layouts)], dtype=B64_ENC_STATE_DTYPE)
            self.rec, self.rec_dtype = mine.tobytes(), B64_ENC_STATE_DTYPE
        self.arena = np.full(scene.dst_len, FILL, dtype=np.uint8).tobytes()

    # -- the records and the arena, out of and back into bytes
    def _states(self):
        sha = np.frombuffer(self.sha, dtype=STATE_DTYPE).copy()
        rec = None if self.rec_dtype is None else np.frombuffer(self.rec, dtype=self.rec_dtype).copy()
        return sha, rec

    def _keep(self, got, sha, rec=None, arena=None):
        self.sha = sha.tobytes()
        got["sha"] = _sha_tuples(sha)
        if rec is not None:
            self.rec = rec.tobytes()
            got["rec"] = _rec_tuples(rec)
        if arena is not None:
            self.arena = arena.tobytes()
            got["arena"] = arena
        return got

    def run(self, k: int) -> dict:
        """Call k on the GPU; what it gave, in the shape piece_cases.check reads."""
        call = self.sc.calls[k]
        if call.fresh:
            self.arena = np.full(self.sc.dst_len, FILL, dtype=np.uint8).tobytes()
        before = None
        if call.switches is not None:
            lines, flat, fused = call.switches
            before = (H.set_b64_lines(lines), H.set_b64_flat(flat), H.set_b64_fused(fused))
        try:
            return getattr(self, "_" + call.route)(call)
        finally:
            if before is not None:
                H.set_b64_lines(before[0])
                H.set_b64_flat(before[1])
                H.set_b64_fused(before[2])

    def run_and_check(self, k: int) -> None:
        P.check(self.sc, k, self.run(k))

    @staticmethod
    def _tables(call):
        return (np.array(call.state_of, dtype=np.uint32), np.array(call.src_off, dtype=np.uint64),
                np.array(call.src_len, dtype=np.uint32), np.array(call.final, dtype=np.uint8), call.expected_array(),
                np.array(call.dst_off, dtype=np.uint64), np.array(call.cap, dtype=np.uint32))

    # -- hash
    def _host_hash(self, call, fn):
        sha, _ = self._states()
        so, off, size, fin, exp, _, _ = self._tables(call)
        verify = call.opts["verify"]
        res = fn(sha, self.sc.src, off, size, state_of=so, final=fin, expected=exp if verify else None)
        return self._keep({"verdicts": res.astype(np.uint8)} if verify else {"digests": res}, sha)

    def _update_chunks(self, call):
        return self._host_hash(call, self.h.update_chunks)

    def _update_chunks_seq(self, call):
        return self._host_hash(call, self.h.update_chunks_seq)

    def _launch_hash(self, call, seq):
        sha, _ = self._states()
        so, off, size, fin, exp, _, _ = self._tables(call)
        n, ns = call.n, self.sc.n_states
        order = np.arange(n)
        if seq:
            order, cs, cf = H.chain_table(so)
        with _Device() as d:
            states, base = d.put(sha), d.put(self.sc.src)
            t = [d.put(a[order]) for a in (off, size, fin, exp)]
            dig, ver = d.filled(20 * n), d.filled(n)
            if seq:
                H.update_seq_launch(states, ns, d.put(cs), d.put(cf), cs.size, base, t[0], t[1], t[2], n, dig, t[3], ver)
            else:
                H.update_launch(states, ns, d.put(so), base, t[0], t[1], t[2], n, dig, t[3], ver)
            H.synchronize()
            got = {"digests": np.empty((n, 20), dtype=np.uint8), "verdicts": np.empty(n, dtype=np.uint8)}
            got["digests"][order] = dig.download(20 * n).reshape(n, 20)
            got["verdicts"][order] = ver.download(n)
            sha = states.download(96 * ns).view(STATE_DTYPE)
        return self._keep(got, sha)

    def _update_launch(self, call):
        return self._launch_hash(call, False)

    def _one_shot_hash(self, call, uniform):
        """lbf_sha1_launch / lbf_sha1_uniform_launch: no records, digests and verdicts only."""
        _, off, size, _, exp, _, _ = self._tables(call)
        n = call.n
        with _Device() as d:
            base, dig, ver = d.put(self.sc.src), d.filled(20 * n), d.filled(n)
            if uniform:
                cs = call.opts["chunk_size"]
                assert (size == cs).all() and (np.diff(off) == cs).all()
                H.uniform_launch(base.ptr + int(off[0]), n * cs, cs, 0, n, dig, d.put(exp), ver)
            else:
                H.batch_launch(base, d.put(off), d.put(size), n, dig, d.put(exp), ver)
            H.synchronize()
            return {"digests": dig.download(20 * n).reshape(n, 20), "verdicts": ver.download(n)}

    def _uniform_launch(self, call):
        return self._one_shot_hash(call, True)

    def _batch_launch(self, call):
        return self._one_shot_hash(call, False)

    def _update_seq_launch(self, call):
        return self._launch_hash(call, True)

    # -- receiver text
    def _host_text(self, call, fn):
        sha, rec = self._states()
        so, off, size, fin, exp, slot, cap = self._tables(call)
        arena = np.frombuffer(self.arena, dtype=np.uint8).copy()
        sizes, ver = fn(rec, sha, self.sc.src, off, size, arena, slot, cap, state_of=so, final=fin, expected=exp)
        return self._keep({"out_sizes": sizes, "verdicts": ver.astype(np.uint8)}, sha, rec, arena)

    def _update_text(self, call):
        return self._host_text(call, self.h.update_text)

    def _update_text_seq(self, call):
        return self._host_text(call, self.h.update_text_seq)

    def _launch_text(self, call, seq):
        sha, rec = self._states()
        so, off, size, fin, exp, slot, cap = self._tables(call)
        n, ns = call.n, self.sc.n_states
        order = np.arange(n)
        if seq:
            order, cs, cf = H.chain_table(so)
        with _Device() as d:
            b64, states, text = d.put(rec), d.put(sha), d.put(self.sc.src)
            out = d.put(np.frombuffer(self.arena, dtype=np.uint8))
            t = {name: d.put(a[order]) for name, a in (("off", off), ("size", size), ("fin", fin), ("exp", exp),
                                                       ("slot", slot), ("cap", cap))}
            osz, dig, ver, poff, psize = d.filled(4 * n), d.filled(20 * n), d.filled(n), d.filled(8 * n), d.filled(4 * n)
            if seq:
                H.b64_update_seq_launch(b64, states, ns, d.put(cs), d.put(cf), cs.size, text, t["off"], t["size"],
                                        t["fin"], n, out, t["slot"], t["cap"], osz, dig, t["exp"], ver, poff, psize)
            else:
                H.b64_update_launch(b64, states, ns, d.put(so), text, t["off"], t["size"], t["fin"], n, out, t["slot"],
                                    t["cap"], osz, dig, t["exp"], ver, poff, psize)
            H.synchronize()
            got = {"digests": np.empty((n, 20), dtype=np.uint8), "verdicts": np.empty(n, dtype=np.uint8),
                   "out_sizes": np.empty(n, dtype=np.uint32)}
            got["digests"][order] = dig.download(20 * n).reshape(n, 20)
            got["verdicts"][order] = ver.download(n)
            got["out_sizes"][order] = osz.download(4 * n).view(np.uint32)
            sha = states.download(96 * ns).view(STATE_DTYPE)
            rec = b64.download(16 * ns).view(B64_STATE_DTYPE)
            arena = out.download(self.sc.dst_len)
        return self._keep(got, sha, rec, arena)

    def _b64_update_launch(self, call):
        return self._launch_text(call, False)

    def _b64_update_seq_launch(self, call):
        return self._launch_text(call, True)

    # -- seeder
    def _update_encode(self, call):
        sha, rec = self._states()
        so, off, size, fin, exp, slot, cap = self._tables(call)
        arena = np.frombuffer(self.arena, dtype=np.uint8).copy()
        noff, nlen, tsz, ver = self.h.update_encode(rec, sha, self.sc.src, off, size, arena, slot, cap, state_of=so,
                                                    final=fin, expected=exp)
        return self._keep({"new_offsets": noff, "new_lens": nlen, "text_sizes": tsz, "verdicts": ver.astype(np.uint8)},
                          sha, rec, arena)

    def _b64_encode_update_launch(self, call):
        sha, rec = self._states()
        so, off, size, fin, exp, slot, cap = self._tables(call)
        n, ns = call.n, self.sc.n_states
        with _Device() as d:
            enc, states, base = d.put(rec), d.put(sha), d.put(self.sc.src)
            text = d.put(np.frombuffer(self.arena, dtype=np.uint8))
            noff, nlen, tsz, dig, ver = d.filled(8 * n), d.filled(4 * n), d.filled(4 * n), d.filled(20 * n), d.filled(n)
            H.b64_encode_update_launch(enc, states, ns, d.put(so), base, d.put(off), d.put(size), d.put(fin), n, text,
                                       d.put(slot), d.put(cap), noff, nlen, tsz, dig, d.put(exp), ver)
            H.synchronize()
            got = {"new_offsets": noff.download(8 * n).view(np.uint64), "new_lens": nlen.download(4 * n).view(np.uint32),
                   "text_sizes": tsz.download(4 * n).view(np.uint32), "digests": dig.download(20 * n).reshape(n, 20),
                   "verdicts": ver.download(n)}
            sha = states.download(96 * ns).view(STATE_DTYPE)
            rec = enc.download(16 * ns).view(B64_ENC_STATE_DTYPE)
            arena = text.download(self.sc.dst_len)
        return self._keep(got, sha, rec, arena)

    # -- one-shot launches
    def _verify_b64_launch(self, call):
        _, off, size, _, exp, slot, cap = self._tables(call)
        n, o = call.n, call.opts
        with _Device() as d:
            out = d.put(np.frombuffer(self.arena, dtype=np.uint8))
            osz, dig, ver, work = d.filled(4 * n), d.filled(20 * n), d.filled(n), d.filled(H.b64_verify_launch_work(n))
            H.verify_b64_launch(d.put(self.sc.src), d.put(off), d.put(size), n, o["max_text_len"], d.put(cap),
                                o["max_size"], out, d.put(slot), osz, work, digests=dig if o["digests"] else None,
                                expected=d.put(exp) if o["verdicts"] else None, verdicts=ver if o["verdicts"] else None)
            H.synchronize()
            return {"out_sizes": osz.download(4 * n).view(np.uint32), "digests": dig.download(20 * n).reshape(n, 20),
                    "verdicts": ver.download(n), "arena": out.download(self.sc.dst_len)}

    def _verify_encode_b64_launch(self, call):
        _, off, size, _, exp, slot, _ = self._tables(call)
        n, o = call.n, call.opts
        with _Device() as d:
            text = d.put(np.frombuffer(self.arena, dtype=np.uint8))
            dig, ver = d.filled(20 * n), d.filled(n)
            H.verify_encode_b64_launch(d.put(self.sc.src), d.put(off), d.put(size), n, o["max_size"], text, d.put(slot),
                                       layout=o["layout"], digests=dig, expected=d.put(exp), verdicts=ver)
            H.synchronize()
            return {"digests": dig.download(20 * n).reshape(n, 20), "verdicts": ver.download(n),
                    "arena": text.download(self.sc.dst_len)}


def run_scene(hasher, scene) -> int:
    """Every call of the scene, each checked; returns the number of calls.  Raises piece_cases.Mismatch."""
    r = Runner(hasher, scene)
    for k in range(len(scene.calls)):
        r.run_and_check(k)
    return len(scene.calls)

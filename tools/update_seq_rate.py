#!/usr/bin/env python3
"""Several pieces of one chain in ONE launch against one launch per piece,
device-resident (diagnostic, not the bench; recorded in DESIGN.md §4.9, not
gated).

C2's shape: 16,384 chains of 256 KiB (lbf_fill_synthetic) in HBM, each fed as
k = 1, 4 and 64 pieces.  One process alternates, round by round,
  hA<k>   route A for the hash: k successive lbf_sha1_update_launch calls, one
          piece per chain each (the last with the final flag)
  hB<k>   route B: one lbf_sha1_update_seq_launch over the k pieces of every chain
and, unless --hash-only, over the chunks' text (--layout xmlrpc: the text
xmlrpc++'s encoder writes, line stage on, flat stage off; --layout flat: the
unbroken text of a Java or Perl peer, both stages on)
  tA<k>       k successive lbf_b64_update_launch calls on the default route
              (lbf_set_b64_fused off)
  tAf<k>      the same on the fused route
  tB<k>       one lbf_b64_update_seq_launch
with HIP events on the launch stream around each case, after a warm-up in
which every case's digests, verdicts, lengths and decoded bytes are checked.
`--rounds` x `--reps` passes per figure.  For each k the result gives B - A of
the medians beside route A's own round-to-round spread (max - min over the
rounds of this run): a difference inside that spread is no difference.

Run it under a time limit:
  timeout -k 10 900 python tools/update_seq_rate.py --out profiles/update_seq/xmlrpc.json
"""
import argparse
import base64
import ctypes
import json
import os
import signal
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bitflood_amd import DeviceBuffer, new_b64_states, new_states  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import check, load  # noqa: E402


def b64_len(size: int) -> int:
    return 4 * (size // 3) + (4 if size % 3 else 0) + size // 3 // 18


def encoder_text(chunk: np.ndarray) -> np.ndarray:
    """xmlrpc++'s text of one chunk: base64, a separator after every 18th complete group."""
    s = np.frombuffer(base64.b64encode(chunk), dtype=np.uint8)
    lines = chunk.size // 3 // 18
    out = np.empty(s.size + lines, dtype=np.uint8)
    body = out[:73 * lines].reshape(lines, 73)
    body[:, :72] = s[:72 * lines].reshape(lines, 72)
    body[:, 72] = ord(" ")
    out[73 * lines:] = s[72 * lines:]
    return out


def flat_len(size: int) -> int:
    return 4 * ((size + 2) // 3)


def flat_text(chunk: np.ndarray) -> np.ndarray:
    """A Java or Perl peer's text of one chunk: RFC 4648, no separators."""
    return np.frombuffer(base64.b64encode(chunk), dtype=np.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--pieces", default="1,4,64", help="pieces per chain, comma-separated")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3, help="passes per case per round")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--hash-only", action="store_true")
    ap.add_argument("--layout", choices=("xmlrpc", "flat"), default="xmlrpc")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, cs = a.chains, a.chunk
    parts = tuple(int(p) for p in a.pieces.split(","))
    lib = load()
    torch.cuda.set_device(0)
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    tl, text_of = (flat_len(cs), flat_text) if a.layout == "flat" else (b64_len(cs), encoder_text)
    slot = (tl + 15) // 16 * 16  # every text 16-byte aligned, as a receiver's frame buffer would be
    kmax = max(parts)
    b = dict(data=DeviceBuffer(n * cs), ref=DeviceBuffer(20 * n), dig=DeviceBuffer(20 * n * kmax),
             sha=DeviceBuffer(96 * n), fin1=DeviceBuffer(n), fin0=DeviceBuffer(n), ver=DeviceBuffer(n * kmax))
    if not a.hash_only:
        b.update(text=DeviceBuffer(n * slot), out=DeviceBuffer(n * cs), b64=DeviceBuffer(16 * n),
                 ooff=DeviceBuffer(8 * n), caps=DeviceBuffer(4 * n), osz=DeviceBuffer(4 * n * kmax),
                 poff=DeviceBuffer(8 * n * kmax), psz=DeviceBuffer(4 * n * kmax))
    try:
        b["data"].fill_synthetic(0x5EED)
        b["sha"].upload(new_states(n))
        b["fin1"].upload(np.ones(n, dtype=np.uint8))
        b["fin0"].upload(np.zeros(n, dtype=np.uint8))
        H.set_kernel_variant(0)
        H.uniform_launch(b["data"], n * cs, cs, 0, n, b["ref"])
        H.synchronize()
        ref = b["ref"].download(20 * n).reshape(n, 20)
        want = ref.tobytes()
        base = np.arange(n, dtype=np.uint64)

        def chain_major(per_piece):
            """per_piece[j] (n entries each) as the table of route B: piece j of chain c at c * k + j."""
            return np.ascontiguousarray(np.stack(per_piece, axis=1)).reshape(-1)

        for p in parts:
            hoff = [base * np.uint64(cs) + np.uint64(k * (cs // p)) for k in range(p)]
            hsz = [np.full(n, cs // p if k < p - 1 else cs - (p - 1) * (cs // p), dtype=np.uint32) for k in range(p)]
            fin = [np.full(n, 1 if k == p - 1 else 0, dtype=np.uint8) for k in range(p)]
            exp = np.zeros((n, p, 20), dtype=np.uint8)
            exp[:, p - 1] = ref
            for k in range(p):  # route A's arrays, one set per launch
                b["hoff", p, k], b["hsz", p, k] = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
                b["hoff", p, k].upload(hoff[k])
                b["hsz", p, k].upload(hsz[k])
            # route B's: the chain table and the same pieces in chain order
            for key, arr in (("first", np.arange(n + 1, dtype=np.uint32) * np.uint32(p)), ("Hoff", chain_major(hoff)),
                             ("Hsz", chain_major(hsz)), ("Fin", chain_major(fin)), ("Exp", exp.reshape(-1))):
                b[key, p] = DeviceBuffer(arr.nbytes)
                b[key, p].upload(arr)
        if not a.hash_only:
            b["b64"].upload(new_b64_states(n))
            b["ooff"].upload(base * np.uint64(cs))
            b["caps"].upload(np.full(n, cs, dtype=np.uint32))
            step = 1024  # chunks per host slice
            for i0 in range(0, n, step):
                m = min(step, n - i0)
                host = b["data"].download(m * cs, offset=i0 * cs)
                text = np.zeros(m * slot, dtype=np.uint8)
                for i in range(m):
                    text[i * slot:i * slot + tl] = text_of(host[i * cs:(i + 1) * cs])
                b["text"].upload(text, offset=i0 * slot)
            for p in parts:  # the text in p parts of (nearly) equal length
                cut = [k * tl // p for k in range(p + 1)]
                toff = [base * np.uint64(slot) + np.uint64(cut[k]) for k in range(p)]
                tlen = [np.full(n, cut[k + 1] - cut[k], dtype=np.uint32) for k in range(p)]
                for k in range(p):
                    b["toff", p, k], b["tlen", p, k] = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
                    b["toff", p, k].upload(toff[k])
                    b["tlen", p, k].upload(tlen[k])
                for key, arr in (("Toff", chain_major(toff)), ("Tlen", chain_major(tlen)),
                                 ("Ooff", np.repeat(base * np.uint64(cs), p)),
                                 ("Caps", np.full(n * p, cs, dtype=np.uint32))):
                    b[key, p] = DeviceBuffer(arr.nbytes)
                    b[key, p].upload(arr)
        stages = (True, a.layout == "flat")  # the line stage, and for unbroken text the flat stage

        def hash_a(p):
            def run():
                for k in range(p):
                    H.update_launch(b["sha"], n, None, b["data"], b["hoff", p, k], b["hsz", p, k],
                                    b["fin1"] if k == p - 1 else b["fin0"], n, b["dig"], b["ref"], b["ver"], stream=sp)
            return run

        def hash_b(p):
            def run():
                H.update_seq_launch(b["sha"], n, None, b["first", p], n, b["data"], b["Hoff", p], b["Hsz", p],
                                    b["Fin", p], n * p, b["dig"], b["Exp", p], b["ver"], stream=sp)
            return run

        def text_a(p, fused):
            def run():
                H.set_b64_lines(stages[0])
                H.set_b64_flat(stages[1])
                H.set_b64_fused(fused)
                for k in range(p):
                    H.b64_update_launch(b["b64"], b["sha"], n, None, b["text"], b["toff", p, k], b["tlen", p, k],
                                        b["fin1"] if k == p - 1 else b["fin0"], n, b["out"], b["ooff"], b["caps"],
                                        b["osz"], b["dig"], b["ref"], b["ver"], b["poff"], b["psz"], stream=sp)
            return run

        def text_b(p):
            def run():
                H.set_b64_lines(stages[0])
                H.set_b64_flat(stages[1])
                H.b64_update_seq_launch(b["b64"], b["sha"], n, None, b["first", p], n, b["text"], b["Toff", p],
                                        b["Tlen", p], b["Fin", p], n * p, b["out"], b["Ooff", p], b["Caps", p],
                                        b["osz"], b["dig"], b["Exp", p], b["ver"], b["poff"], b["psz"], stream=sp)
            return run

        # (name, what to run, pieces per chain, results at c * k + k - 1 rather than at c)
        cases = []
        for p in parts:
            cases += [(f"hA{p}", hash_a(p), p, False), (f"hB{p}", hash_b(p), p, True)]
        if not a.hash_only:
            for p in parts:
                cases += [(f"tA{p}", text_a(p, False), p, False), (f"tAf{p}", text_a(p, True), p, False),
                          (f"tB{p}", text_b(p), p, True)]
        probe = min(64 << 20, n * cs)  # the part of the decoded bytes that is compared with the chunks
        ms = {name: [] for name, *_ in cases}
        agree = {}
        fused_before = H.set_b64_fused(False)

        def timed(fn, reps):
            signal.alarm(a.step_timeout)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            signal.alarm(0)
            return e0.elapsed_time(e1) / reps

        for name, fn, p, seq in cases:  # warm-up, and every case's results
            m = n * p if seq else n
            b["dig"].upload(np.zeros(20 * m, dtype=np.uint8))
            b["ver"].upload(np.zeros(m, dtype=np.uint8))
            if name.startswith("t"):
                b["osz"].upload(np.zeros(m, dtype=np.uint32))
                b["out"].upload(np.zeros(probe, dtype=np.uint8))
            timed(fn, 1)
            at = slice(p - 1, None, p) if seq else slice(None)  # the final pieces' entries
            ok = b["dig"].download(20 * m).reshape(m, 20)[at].tobytes() == want and bool(b["ver"].download(m)[at].all())
            if name.startswith("t"):
                ok = ok and bool((b["osz"].download(4 * m, dtype=np.uint32)[at] == cs).all())
                ok = ok and b["out"].download(probe).tobytes() == b["data"].download(probe).tobytes()
            ok = ok and b["sha"].download(96 * n).tobytes() == new_states(n).tobytes()
            agree[name] = ok
        for _ in range(a.rounds):
            for name, fn, _, _ in cases:
                ms[name].append(timed(fn, a.reps))
        H.set_b64_fused(fused_before)
        gib = n * cs / 2**30
        res = {"mode": "hash-only" if a.hash_only else "text", "layout": a.layout, "chains": n, "chunk": cs,
               "text_chars": tl, "gib": gib, "rounds": a.rounds, "reps": a.reps,
               "library": os.environ.get("LBF_LIB", "in-tree"), "cases": {}, "b_against_a": {}}
        for name, _, p, _ in cases:
            v = [x * 4 / gib for x in ms[name]]
            res["cases"][name] = {"pieces_per_chain": p, "ms_per_4gib_median": round(statistics.median(v), 4),
                                  "ms_min": round(min(v), 4), "ms_max": round(max(v), 4),
                                  "spread_ms": round(max(v) - min(v), 4), "results_agree": agree[name]}
        pairs = [("hB", "hA")] + ([] if a.hash_only else [("tB", "tA"), ("tB", "tAf")])
        for p in parts:
            for bn, an in pairs:
                ca, cb = res["cases"][f"{an}{p}"], res["cases"][f"{bn}{p}"]
                diff = round(cb["ms_per_4gib_median"] - ca["ms_per_4gib_median"], 4)
                res["b_against_a"][f"{bn}{p}-{an}{p}"] = {
                    "ms_per_4gib": diff, "a_spread_ms": ca["spread_ms"],
                    "verdict": "level" if abs(diff) <= ca["spread_ms"] else ("B faster" if diff < 0 else "B slower")}
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if all(agree.values()) else 1
    finally:
        for buf in b.values():
            buf.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

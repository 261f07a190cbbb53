#!/usr/bin/env python3
"""Rate of the piecewise base64 decode chained to the resumable SHA-1
(lbf_b64_update_launch), device-resident (diagnostic, not the bench; recorded
in DESIGN.md §4.7 and §5, not gated).

C2's shape: 16,384 chunks of 256 KiB (lbf_fill_synthetic) as the text
xmlrpc++'s encoder writes for them (--layout xmlrpc: 354,382 characters a
chunk) or as the unbroken text a Java or Perl peer sends (--layout flat:
349,528), built on the host slice by slice and uploaded.  One process
alternates, round by round,
  t1_flat, t1_lines, t1_flatonly, t1_scan
                       the text as one piece with the final flag, on four
                       routes: line and flat path on (one launch = five
                       kernels), the line path alone (four; the default route),
                       the flat path alone (four), and neither (three)
  t1_fused, t1_fusedlines
                       the same on the fused route (lbf_set_b64_fused: three
                       kernels whatever the stage mask): line and flat stage on,
                       and the line stage alone
  t4_*                 four pieces of a quarter of the text each
  t64_*                64 pieces
  h1, h4, h64   lbf_sha1_update_launch alone over the decoded bytes, cut the same way
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` passes per figure; t - h is the decode's share,
and a case's spread is its max - min over the rounds.  After the warm-up every
verdict must be 1, every decoded length the chunk size, and the decoded bytes
the chunks.  Also reported: the share of each case's characters that the line
path takes (a sample of the chains through lbf_b64_update_batch, whose context
counts them), and what each path's enqueue costs a call (launches of
empty pieces, route against route, alternating).

  --one-shot         lbf_b64_verify_batch over 1,024 of the texts, the flat
                     path on and off alternating: the whole host call is timed
                     (the text's H2D included); the decode kernels' own times
                     are read from a kernel trace, as for --general-decode

Comparators from another build of the library (LBF_LIB=<its liblbfhash.so>):
  --hash-only        h1, h4, h64 alone (a library without the text entry points)
  --general-decode   lbf_b64_verify_batch over 1,024 of the texts with one junk
                     character in front of each, so that the general two-pass
                     b64_decode_kernel takes them; the whole host call is timed,
                     and the kernel's own time is read from a kernel trace
                     (rocprofv3 --kernel-trace --stats -- python tools/wire_update_rate.py ...)

Run it under a time limit:
  timeout -k 10 600 python tools/wire_update_rate.py --out profiles/wire_update_rate.json
"""
import argparse
import base64
import ctypes
import json
import os
import signal
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bitflood_amd import ChunkHasher, DeviceBuffer, new_b64_states, new_states  # noqa: E402
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


def one_shot(a):
    """lbf_b64_verify_batch on whole texts of the chosen layout, the flat path on and off in turn."""
    import hashlib
    n, cs = min(a.chains, 1024), a.chunk
    dev = DeviceBuffer(n * cs)
    dev.fill_synthetic(0x5EED)
    H.synchronize()
    data = dev.download(n * cs)
    dev.free()
    tl, text_of = (flat_len(cs), flat_text) if a.layout == "flat" else (b64_len(cs), encoder_text)
    slot = (tl + 15) // 16 * 16
    text = np.zeros(slot * n, dtype=np.uint8)
    for i in range(n):
        text[i * slot:i * slot + tl] = text_of(data[i * cs:(i + 1) * cs])
    exp = np.frombuffer(b"".join(hashlib.sha1(data[i * cs:(i + 1) * cs]).digest() for i in range(n)), np.uint8)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(slot)
    out = np.zeros(n * cs, dtype=np.uint8)
    ooff = np.arange(n, dtype=np.uint64) * np.uint64(cs)
    ms, counts, ok = {"flat_on": [], "flat_off": []}, {}, True
    with ChunkHasher(device_mask=1) as h:
        for on in (True, False):
            H.set_b64_flat(on)
            h.verify_b64(text, toff, np.full(n, tl), np.full(n, cs), exp, out, ooff)  # warm-up, scratch grown
        for _ in range(a.rounds):
            for name, on in (("flat_on", True), ("flat_off", False)):
                H.set_b64_flat(on)
                out[:] = 0
                s0, f0 = h.b64_stats(), h.b64_flat_stats()
                t0 = time.perf_counter()
                for _ in range(a.reps):
                    ver, dec = h.verify_b64(text, toff, np.full(n, tl), np.full(n, cs), exp, out, ooff)
                ms[name].append((time.perf_counter() - t0) / a.reps * 1e3)
                s1, f1 = h.b64_stats(), h.b64_flat_stats()
                counts[name] = {"one_pass": (s1["one_pass"] - s0["one_pass"]) // a.reps,
                                "general": (s1["general"] - s0["general"]) // a.reps,
                                "flat_chunks": (f1["flat_chunks"] - f0["flat_chunks"]) // a.reps}
                ok = ok and bool(ver.all() and (dec == cs).all() and np.array_equal(out, data))
    want_flat = n if a.layout == "flat" else 0
    ok = ok and counts["flat_on"]["flat_chunks"] == want_flat and counts["flat_off"]["flat_chunks"] == 0
    res = {"mode": "one-shot", "layout": a.layout, "chunks": n, "chunk": cs, "text_chars": tl, "rounds": a.rounds,
           "reps": a.reps, "parity": ok, "chunks_by_path": counts,
           "host_call_ms": {k: {"median": round(statistics.median(v), 3), "min": round(min(v), 3),
                                "max": round(max(v), 3)} for k, v in ms.items()}}
    return res, ok


def general_decode(a):
    """The comparator for the decode: the general kernel through the host call."""
    n, cs = min(a.chains, 1024), a.chunk
    dev = DeviceBuffer(n * cs)
    dev.fill_synthetic(0x5EED)
    H.synchronize()
    data = dev.download(n * cs)
    dev.free()
    tl = b64_len(cs) + 1
    slot = (tl + 15) // 16 * 16
    text = np.zeros(slot * n, dtype=np.uint8)
    for i in range(n):
        text[i * slot] = ord("*")  # outside the encoder's layout: the one-pass decode hands the text on
        text[i * slot + 1:i * slot + tl] = encoder_text(data[i * cs:(i + 1) * cs])
    import hashlib
    exp = np.frombuffer(b"".join(hashlib.sha1(data[i * cs:(i + 1) * cs]).digest() for i in range(n)), np.uint8)
    toff = np.arange(n, dtype=np.uint64) * np.uint64(slot)
    out = np.zeros(n * cs, dtype=np.uint8)
    ooff = np.arange(n, dtype=np.uint64) * np.uint64(cs)
    with ChunkHasher(device_mask=1) as h:
        h.verify_b64(text, toff, np.full(n, tl), np.full(n, cs), exp, out, ooff)
        before = h.b64_stats()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            ver, dec = h.verify_b64(text, toff, np.full(n, tl), np.full(n, cs), exp, out, ooff)
        dt = (time.perf_counter() - t0) / a.reps
        after = h.b64_stats()
    res = {"mode": "general-decode", "chunks": n, "chunk": cs, "calls": a.reps, "host_call_ms": round(dt * 1e3, 3),
           "general_chunks_per_call": (after["general"] - before["general"]) // a.reps,
           "parity": bool(ver.all() and (dec == cs).all() and np.array_equal(out, data))}
    return res, res["parity"] and res["general_chunks_per_call"] == n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=4, help="passes per case per round")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--hash-only", action="store_true")
    ap.add_argument("--general-decode", action="store_true")
    ap.add_argument("--one-shot", action="store_true")
    ap.add_argument("--layout", choices=("xmlrpc", "flat"), default="xmlrpc")
    ap.add_argument("--cases", default="", help="comma-separated subset of the cases (for a kernel trace of one)")
    ap.add_argument("--share-chains", type=int, default=64, help="chains of the line-share sample")
    ap.add_argument("--empty-reps", type=int, default=200, help="empty launches per round of the enqueue cost")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n, cs = a.chains, a.chunk
    lib = load()
    torch.cuda.set_device(0)

    def emit(res, ok):
        res["library"] = os.environ.get("LBF_LIB", "in-tree")
        res.setdefault("layout", a.layout)
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if ok else 1

    if a.general_decode:
        return emit(*general_decode(a))
    if a.one_shot:
        return emit(*one_shot(a))

    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    tl, text_of = (flat_len(cs), flat_text) if a.layout == "flat" else (b64_len(cs), encoder_text)
    slot = (tl + 15) // 16 * 16  # every text 16-byte aligned, as a receiver's frame buffer would be
    parts = (1, 4, 64)
    bufs = dict(data=DeviceBuffer(n * cs), ref=DeviceBuffer(20 * n), dig=DeviceBuffer(20 * n), sha=DeviceBuffer(96 * n),
                fin1=DeviceBuffer(n), fin0=DeviceBuffer(n), ver=DeviceBuffer(n))
    if not a.hash_only:
        bufs.update(text=DeviceBuffer(n * slot), out=DeviceBuffer(n * cs), b64=DeviceBuffer(16 * n),
                    ooff=DeviceBuffer(8 * n), caps=DeviceBuffer(4 * n), osz=DeviceBuffer(4 * n),
                    poff=DeviceBuffer(8 * n), psz=DeviceBuffer(4 * n))
    try:
        b = bufs
        b["data"].fill_synthetic(0x5EED)
        b["sha"].upload(new_states(n))
        b["fin1"].upload(np.ones(n, dtype=np.uint8))
        b["fin0"].upload(np.zeros(n, dtype=np.uint8))
        H.set_kernel_variant(0)
        H.uniform_launch(b["data"], n * cs, cs, 0, n, b["ref"])
        H.synchronize()
        want = b["ref"].download(20 * n).tobytes()
        base = np.arange(n, dtype=np.uint64)
        for p in parts:  # the hash comparator's pieces: the chunk's bytes in p equal parts
            b["hsz", p] = DeviceBuffer(4 * n)
            b["hsz", p].upload(np.full(n, cs // p, dtype=np.uint32))
            for k in range(p):
                b["hoff", p, k] = DeviceBuffer(8 * n)
                b["hoff", p, k].upload(base * np.uint64(cs) + np.uint64(k * (cs // p)))
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
                for k in range(p):
                    b["toff", p, k], b["tlen", p, k] = DeviceBuffer(8 * n), DeviceBuffer(4 * n)
                    b["toff", p, k].upload(base * np.uint64(slot) + np.uint64(cut[k]))
                    b["tlen", p, k].upload(np.full(n, cut[k + 1] - cut[k], dtype=np.uint32))
            b["tlen0"] = DeviceBuffer(4 * n)
            b["tlen0"].upload(np.zeros(n, dtype=np.uint32))
        # (route, line path, flat path, fused route); a library from before a path or the fused route (LBF_LIB) has
        # fewer routes
        if hasattr(lib, "lbf_set_b64_flat"):
            off = False if hasattr(lib, "lbf_set_b64_fused") else None
            routes = (("flat", True, True, off), ("lines", True, False, off), ("flatonly", False, True, off),
                      ("scan", False, False, off))
            if off is not None:
                routes += (("fused", True, True, True), ("fusedlines", True, False, True))
        elif hasattr(lib, "lbf_set_b64_lines"):
            routes = (("lines", True, None, None), ("scan", False, None, None))
        else:
            routes = (("scan", None, None, None),)

        def set_route(lines, flat, fused):
            if lines is not None:
                H.set_b64_lines(lines)
            if flat is not None:
                H.set_b64_flat(flat)
            if fused is not None:
                H.set_b64_fused(fused)

        def text_pieces(p, *route):
            def run():
                set_route(*route)
                for k in range(p):
                    H.b64_update_launch(b["b64"], b["sha"], n, None, b["text"], b["toff", p, k], b["tlen", p, k],
                                        b["fin1"] if k == p - 1 else b["fin0"], n, b["out"], b["ooff"], b["caps"],
                                        b["osz"], b["dig"], b["ref"], b["ver"], b["poff"], b["psz"], stream=sp)
            return run

        def hash_pieces(p):
            def run():
                # the bytes the decode wrote, once a text case has run; the chunks themselves otherwise
                src = b["out"] if decoded_once else b["data"]
                for k in range(p):
                    H.update_launch(b["sha"], n, None, src, b["hoff", p, k], b["hsz", p],
                                    b["fin1"] if k == p - 1 else b["fin0"], n, b["dig"], b["ref"], b["ver"], stream=sp)
            return run

        def empty_launch(*route):
            def run():
                set_route(*route)
                H.b64_update_launch(b["b64"], b["sha"], n, None, b["text"], b["toff", 1, 0], b["tlen0"], b["fin0"], n,
                                    b["out"], b["ooff"], b["caps"], b["osz"], b["dig"], b["ref"], b["ver"], b["poff"],
                                    b["psz"], stream=sp)
            return run

        def line_share(p, route):
            """The line and flat paths' shares of the characters of case t<p> on `route`: the first chains
            through the batch call."""
            m = min(a.share_chains, n)
            text = b["text"].download(m * slot)
            cut = [k * tl // p for k in range(p + 1)]
            b64s, shas = new_b64_states(m), new_states(m)
            out = np.zeros(m * cs, dtype=np.uint8)
            set_route(*route)
            with ChunkHasher(device_mask=1) as h:
                for k in range(p):
                    h.update_text(b64s, shas, text, np.arange(m) * slot + cut[k], np.full(m, cut[k + 1] - cut[k]), out,
                                  np.arange(m) * cs, np.full(m, cs), final=np.full(m, k == p - 1))
                st = h.b64_update_stats()
                flat = h.b64_flat_stats()["flat_chars"] if hasattr(lib, "lbf_set_b64_flat") else 0
            assert st["line_chars"] + st["scan_chars"] == m * tl and flat <= st["scan_chars"], (st, flat)
            return {"line": round(st["line_chars"] / (m * tl), 6), "flat": round(flat / (m * tl), 6)}

        cases = [] if a.hash_only else [(f"t{p}_{route}", text_pieces(p, *how), p) for p in parts
                                         for route, *how in routes]
        cases += [(f"h{p}", hash_pieces(p), p) for p in parts]
        if a.cases:
            want = a.cases.split(",")  # "t4" names both of its routes, "t4_lines" one
            cases = [c for c in cases if c[0] in want or c[0].split("_")[0] in want]
        decoded_once = any(name.startswith("t") for name, _, _ in cases)  # the t cases come first
        probe = min(64 << 20, n * cs)  # the part of the decoded bytes that is compared with the chunks
        ms = {name: [] for name, _, _ in cases}
        agree = {}

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

        for name, fn, _ in cases:  # warm-up, and every case's results
            b["dig"].upload(np.zeros(20 * n, dtype=np.uint8))
            b["ver"].upload(np.zeros(n, dtype=np.uint8))
            if name.startswith("t"):
                b["osz"].upload(np.zeros(n, dtype=np.uint32))
                b["out"].upload(np.zeros(probe, dtype=np.uint8))
            timed(fn, 1)
            ok = b["dig"].download(20 * n).tobytes() == want and bool(b["ver"].download(n).all())
            if name.startswith("t"):
                ok = ok and bool((b["osz"].download(4 * n, dtype=np.uint32) == cs).all())
                ok = ok and b["out"].download(probe).tobytes() == b["data"].download(probe).tobytes()
            agree[name] = ok
        for _ in range(a.rounds):
            for name, fn, _ in cases:
                ms[name].append(timed(fn, a.reps))
        gib = n * cs / 2**30
        res = {"mode": "hash-only" if a.hash_only else "text", "chains": n, "chunk": cs, "text_chars": tl,
               "gib_decoded": gib, "rounds": a.rounds, "reps": a.reps, "cases": {}}
        for name, _, launches in cases:
            med = statistics.median(ms[name])
            res["cases"][name] = {"launches_per_pass": launches, "ms_per_4gib_median": round(med * 4 / gib, 4),
                                  "ms_min": round(min(ms[name]) * 4 / gib, 4),
                                  "ms_max": round(max(ms[name]) * 4 / gib, 4),
                                  "spread_ms": round((max(ms[name]) - min(ms[name])) * 4 / gib, 4),
                                  "results_agree": agree[name]}
        if not a.hash_only and not a.cases:
            res["decode_share_ms"] = {f"t{p}_{route}": round(res["cases"][f"t{p}_{route}"]["ms_per_4gib_median"] -
                                                              res["cases"][f"h{p}"]["ms_per_4gib_median"], 4)
                                      for p in parts for route, *_ in routes}
            if len(routes) >= 2:
                res["share_of_chars"] = {f"t{p}": line_share(p, routes[0][1:]) for p in parts}
                if len(routes) > 4:  # the same characters by the same paths on the fused route
                    res["share_of_chars_fused"] = {f"t{p}": line_share(p, routes[4][1:]) for p in parts}
                us = {route: [] for route, *_ in routes}
                for _, *how in routes:
                    timed(empty_launch(*how), 10)
                for _ in range(a.rounds):
                    for route, *how in routes:
                        us[route].append(timed(empty_launch(*how), a.empty_reps) * 1e3)
                med = {r: statistics.median(v) for r, v in us.items()}
                res["empty_launch_us"] = {"pieces": n}
                for r, v in us.items():
                    res["empty_launch_us"][r] = {"median": round(med[r], 3), "min": round(min(v), 3),
                                                 "max": round(max(v), 3)}
                res["empty_launch_us"]["lines_enqueue_us_per_call"] = round(med["lines"] - med["scan"], 3)
                if "flat" in med:
                    res["empty_launch_us"]["flat_enqueue_us_per_call"] = round(med["flat"] - med["lines"], 3)
                if "fused" in med:
                    res["empty_launch_us"]["fused_saves_us_per_call"] = round(med["flat"] - med["fused"], 3)
                    res["empty_launch_us"]["fusedlines_saves_us_per_call"] = round(med["lines"] - med["fusedlines"], 3)
        return emit(res, all(agree.values()))
    finally:
        for buf in bufs.values():
            buf.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""What the flood file's hash strings cost on the device: lbf_sha1_hashes_launch
and lbf_verify_hashes_launch against lbf_sha1_launch alone (diagnostic, not the
bench; recorded in DESIGN.md §4.10 and §5, not gated).

C2's shape in HBM: 16,384 chunks of 256 KiB (lbf_fill_synthetic).  One process
alternates, round by round,
  sha1                       lbf_sha1_launch with binary expected digests and
                             verdicts: the route the new launches replace,
                             minus its host work on either side
  hashes                     lbf_sha1_hashes_launch, packed slots
  verify_good, verify_bad    lbf_verify_hashes_launch without the list, every
                             hash right / every third hash damaged
  verify_good_list, verify_bad_list   the same with d_missing / d_missing_count
with HIP events on the launch stream around each case's launches, after a
warm-up, `--rounds` x `--reps` passes per figure.  A case's spread is its
max - min over the rounds; extra_over_sha1_us is its median minus sha1's, to be
read next to sha1's own spread.

The kernels alone, where the hash is next to nothing: the same cases over
`--tiny-chains` (262,144) chunks of one byte (tiny_*), and over the same count
with the digests precomputed (kernels_*: the library's internal launchers
behind the hash, found by name in the shared object; null where it exports
none).

In the warm-up every case's results must be the CPU's: base64 of hashlib's
SHA-1 for the strings, '1' / '0' by the damage for the chunkmap, the damaged
indices ascending for the list.

Run it under a time limit:
  timeout -k 10 600 python tools/hash_text_rate.py --out profiles/hash_text/rate.json
"""
import argparse
import base64
import ctypes
import hashlib
import json
import os
import signal
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from bitflood_amd import DeviceBuffer, verify_hashes_launch_work  # noqa: E402
from bitflood_amd import hashing as H  # noqa: E402
from bitflood_amd._capi import LIB_PATH, check, load  # noqa: E402


class _Verify(ctypes.Structure):  # hash_text.hpp's HashTextVerify
    _fields_ = [(k, ctypes.c_void_p) for k in ("digests", "hashes", "hash_off", "hash_len", "chunkmap", "counts",
                                               "missing", "missing_count")] + [("n", ctypes.c_uint32)]


def internal_launchers(lib):
    """hash_text.hpp's two launchers by their mangled names, or (None, None)."""
    out = subprocess.run(["nm", "-D", "--defined-only", LIB_PATH], capture_output=True, text=True, check=True).stdout
    names = [line.split()[-1] for line in out.splitlines() if "launch_hash_text_" in line]
    enc = [s for s in names if "launch_hash_text_encode" in s]
    ver = [s for s in names if "launch_hash_text_verify" in s]
    if len(enc) != 1 or len(ver) != 1:
        return None, None
    e, v = getattr(lib, enc[0]), getattr(lib, ver[0])
    e.restype = v.restype = ctypes.c_int
    e.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_uint32, ctypes.c_void_p]
    v.argtypes = [ctypes.POINTER(_Verify), ctypes.c_void_p]
    return e, v


class Shape:
    """n chunks of `size` bytes back to back in HBM, their tables, the strings
    right and damaged, and one set of outputs."""

    def __init__(self, n, size, seed):
        self.n, self.size = n, size
        self.b = b = dict(data=DeviceBuffer((n * size + 15) // 16 * 16), off=DeviceBuffer(8 * n),
                          size=DeviceBuffer(4 * n), ref=DeviceBuffer(20 * n), dig=DeviceBuffer(20 * n),
                          ver=DeviceBuffer(n), good=DeviceBuffer(27 * n), bad=DeviceBuffer(27 * n),
                          out=DeviceBuffer(27 * n), cmap=DeviceBuffer(n), miss=DeviceBuffer(4 * n),
                          cnt=DeviceBuffer(4), work=DeviceBuffer(verify_hashes_launch_work(n)))
        b["data"].fill_synthetic(seed)
        b["off"].upload(np.arange(n, dtype=np.uint64) * np.uint64(size))
        b["size"].upload(np.full(n, size, dtype=np.uint32))
        H.batch_launch(b["data"], b["off"], b["size"], n, b["ref"])
        H.synchronize()
        self.digests = b["ref"].download(20 * n).reshape(n, 20)
        self.strings = np.frombuffer(b"".join(base64.b64encode(d.tobytes())[:27] for d in self.digests),
                                     np.uint8).reshape(n, 27).copy()
        damaged = self.strings.copy()
        damaged[::3, 0] = np.where(damaged[::3, 0] == ord("A"), ord("B"), ord("A"))
        b["good"].upload(self.strings)
        b["bad"].upload(damaged)
        self.bad_idx = np.arange(0, n, 3, dtype=np.uint32)

    def probe(self, m):
        """hashlib over the first m chunks against the library's digests."""
        host = self.b["data"].download(m * self.size)
        return all(hashlib.sha1(host[i * self.size:(i + 1) * self.size].tobytes()).digest() == self.digests[i].tobytes()
                   for i in range(m))

    def free(self):
        for buf in self.b.values():
            buf.free()


def cases_of(s, sp, prefix, enc, ver):
    """(name, launch, check) for one shape; enc/ver given: the kernels behind the hash alone."""
    b, n = s.b, s.n

    def clear():
        b["out"].upload(np.zeros(27 * n, np.uint8))
        b["cmap"].upload(np.zeros(n, np.uint8))
        b["miss"].upload(np.full(n, 0xFFFFFFFF, np.uint32))
        b["cnt"].upload(np.full(1, 0xFFFFFFFF, np.uint32))
        b["ver"].upload(np.zeros(n, np.uint8))

    def sha1():
        H.batch_launch(b["data"], b["off"], b["size"], n, b["dig"], b["ref"], b["ver"], stream=sp)

    def hashes():
        if enc:
            check(enc(b["ref"].ptr, b["out"].ptr, None, n, sp))
        else:
            H.sha1_hashes_launch(b["data"], b["off"], b["size"], n, b["out"], b["work"], stream=sp)

    def verify(which, listed):
        def run():
            if ver:
                counts = b["work"].ptr + ((20 * n + 15) & ~15)
                v = _Verify(b["ref"].ptr, b[which].ptr, None, None, b["cmap"].ptr, counts if listed else None,
                            b["miss"].ptr if listed else None, b["cnt"].ptr if listed else None, n)
                check(ver(ctypes.byref(v), sp))
            else:
                H.verify_hashes_launch(b["data"], b["off"], b["size"], n, b[which], b["cmap"], b["work"],
                                       missing=b["miss"] if listed else None,
                                       missing_count=b["cnt"] if listed else None, stream=sp)
        return run

    def ok_sha1():
        return bool(b["ver"].download(n).all()) and np.array_equal(b["dig"].download(20 * n).reshape(n, 20), s.digests)

    def ok_hashes():
        return np.array_equal(b["out"].download(27 * n).reshape(n, 27), s.strings)

    def ok_verify(which, listed):
        def ok():
            want = np.full(n, ord("1"), np.uint8)
            idx = s.bad_idx if which == "bad" else s.bad_idx[:0]
            want[idx] = ord("0")
            good = np.array_equal(b["cmap"].download(n), want)
            if listed:
                miss = b["miss"].download(4 * n, dtype=np.uint32)
                good = good and int(b["cnt"].download(dtype=np.uint32)[0]) == len(idx)
                good = good and np.array_equal(miss[:len(idx)], idx) and bool((miss[len(idx):] == 0xFFFFFFFF).all())
            return bool(good)
        return ok

    out = [] if enc or ver else [(prefix + "sha1", sha1, ok_sha1)]
    out.append((prefix + "hashes", hashes, ok_hashes))
    for which in ("good", "bad"):
        for listed in (False, True):
            out.append((f"{prefix}verify_{which}{'_list' if listed else ''}", verify(which, listed),
                        ok_verify(which, listed)))
    return [(name, fn, ok, clear) for name, fn, ok in out]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chains", type=int, default=16384)
    ap.add_argument("--chunk", type=int, default=262144)
    ap.add_argument("--tiny-chains", type=int, default=262144)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=4, help="passes per case per round at C2's shape")
    ap.add_argument("--tiny-reps", type=int, default=20, help="passes per case per round of the one-byte chunks")
    ap.add_argument("--step-timeout", type=int, default=120, help="seconds one case of one round may take")
    ap.add_argument("--probe-chunks", type=int, default=16, help="chunks hashed again by hashlib")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    lib = load()
    torch.cuda.set_device(0)
    sp = ctypes.c_void_p()
    check(lib.lbf_stream_create(ctypes.byref(sp)))
    stream = torch.cuda.ExternalStream(sp.value)
    H.set_kernel_variant(0)
    shapes = []
    try:
        c2, tiny = Shape(a.chains, a.chunk, 0x5EED), Shape(a.tiny_chains, 1, 0x5EED)
        shapes += [c2, tiny]
        hashlib_agrees = c2.probe(min(a.probe_chunks, c2.n)) and tiny.probe(min(a.probe_chunks, tiny.n))
        enc, ver = internal_launchers(lib)
        groups = [(cases_of(c2, sp, "", None, None), a.reps), (cases_of(tiny, sp, "tiny_", None, None), a.tiny_reps)]
        if enc and ver:
            groups.append((cases_of(tiny, sp, "kernels_", enc, ver), a.tiny_reps))

        def timed(fn, reps):
            signal.alarm(a.step_timeout)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record(stream)
            for _ in range(reps):
                fn()
            e1.record(stream)
            e1.synchronize()
            signal.alarm(0)
            return e0.elapsed_time(e1) * 1000.0 / reps  # us a pass

        us, agree = {}, {}
        for cases, _ in groups:  # warm-up, and every case's results
            for name, fn, ok, clear in cases:
                clear()
                timed(fn, 1)
                agree[name], us[name] = ok(), []
        for _ in range(a.rounds):
            for cases, reps in groups:
                for name, fn, _, _ in cases:
                    us[name].append(timed(fn, reps))
        res = {"mode": "hash-text-rate", "chains": c2.n, "chunk": c2.size, "tiny_chains": tiny.n, "rounds": a.rounds,
               "reps": a.reps, "tiny_reps": a.tiny_reps, "library": os.environ.get("LBF_LIB", "in-tree"),
               "hash_kernel": {"c2": lib.lbf_kernel_for(c2.n), "tiny": lib.lbf_kernel_for(tiny.n)},
               "hashlib_agrees": hashlib_agrees, "kernels_alone_measured": bool(enc and ver), "cases": {}}
        for name, v in us.items():
            res["cases"][name] = {"us_median": round(statistics.median(v), 2), "us_min": round(min(v), 2),
                                  "us_max": round(max(v), 2), "spread_us": round(max(v) - min(v), 2),
                                  "results_agree": agree[name]}
        for prefix in ("", "tiny_"):
            base = res["cases"][prefix + "sha1"]
            res[prefix + "extra_over_sha1_us"] = {
                name: round(c["us_median"] - base["us_median"], 2) for name, c in res["cases"].items()
                if name.startswith(prefix + "hashes") or name.startswith(prefix + "verify_")}
            res[prefix + "sha1_spread_us"] = base["spread_us"]
        line = json.dumps(res)
        print(line, flush=True)
        if a.out:
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return 0 if hashlib_agrees and all(agree.values()) else 1
    finally:
        for s in shapes:
            s.free()
        check(lib.lbf_stream_destroy(sp))


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Merge one lease's runs of tools/wire_update_rate.py into the document kept
as profiles/wire_update_rate.json (no GPU needed).

The runs, all on one lease, into one directory DIR:
  python tools/wire_update_rate.py --out DIR/new.json
  LBF_LIB=<parent commit's liblbfhash.so> python tools/wire_update_rate.py --hash-only --out DIR/parent_hash.json
  for c in t1 t4 t64:
    rocprofv3 --kernel-trace --stats -d DIR/trace_$c -o trace --output-format csv -- \\
        python tools/wire_update_rate.py --cases $c --rounds 2 --reps 4
  LBF_LIB=<parent's> rocprofv3 --kernel-trace --stats -d DIR/trace_general -o trace --output-format csv -- \\
        python tools/wire_update_rate.py --general-decode --reps 5 --out DIR/parent_general.json
Then:
  python tools/wire_update_summary.py DIR profiles/wire_update_rate.json

`kernel_trace` holds each kernel's own duration from the stats files (average,
minimum, maximum in microseconds, warm-up launches included) and
`ms_per_4gib`, the average times the case's launches per pass; the general
decode runs 1,024 chunks a launch, a sixteenth of 4 GiB.
"""
import csv
import glob
import json
import os
import sys

KERNELS = ("b64_update_lines_kernel", "b64_update_kernel", "sha1_update_kernel", "b64_length_kernel", "b64_decode_kernel",
           "b64_decode_canon_kernel")
LAUNCHES = {"t1": 1, "t4": 4, "t64": 64}


def stats(directory):
    """{kernel: calls and microseconds} from the *kernel_stats.csv under `directory`."""
    found = sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True))
    if not found:
        raise SystemExit(f"no kernel_stats.csv under {directory}")
    out = {}
    with open(found[0]) as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if "::" + k + "(" in row["Name"]:
                    out[k] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2),
                              "min_us": round(int(row["MinNs"]) / 1e3, 2), "max_us": round(int(row["MaxNs"]) / 1e3, 2)}
    return out


def run_line(path):
    with open(path) as f:
        res = json.loads(f.read())
    res["library"] = "in-tree" if res.get("library") == "in-tree" else "parent commit"  # no paths in the record
    return res


def main():
    if len(sys.argv) != 3:
        raise SystemExit(__doc__)
    d, dest = sys.argv[1], sys.argv[2]
    trace = {}
    for case, launches in LAUNCHES.items():
        s = stats(os.path.join(d, "trace_" + case))
        s["ms_per_4gib"] = {k: round(v["avg_us"] * launches / 1e3, 3) for k, v in s.items()}
        trace[case] = s
    general = stats(os.path.join(d, "trace_general"))
    general["chunks_per_launch"] = 1024
    general["b64_decode_kernel_ms_per_4gib"] = round(general["b64_decode_kernel"]["avg_us"] * 16 / 1e3, 3)
    res = {"tool": "tools/wire_update_rate.py, merged by tools/wire_update_summary.py",
           "note": "one lease; events: 5 rounds x 4 passes per case, median ms per 4 GiB decoded; traces: rocprofv3 "
                   "--kernel-trace --stats of one case each (--rounds 2 --reps 4, warm-up included)",
           "text": run_line(os.path.join(d, "new.json")),
           "parent_hash_only": run_line(os.path.join(d, "parent_hash.json")),
           "kernel_trace": trace,
           "parent_general_decode": {"host_call": run_line(os.path.join(d, "parent_general.json")),
                                     "kernel_trace": general}}
    with open(dest, "w") as f:
        f.write(json.dumps(res, indent=1) + "\n")
    print(dest)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Per-call durations of chosen kernels from a `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python bench.py ...` run:
    python3 profiles/kcalls.py DIR [substring of a kernel's name ...]
one line per kernel (calls, mean, min-max in microseconds) and the sum over all dispatches of the process.  Without substrings: the
kernels of the k-mer build's cut (profiles/r08_part_records.md)."""
import csv
import glob
import sys

d = sys.argv[1]
want = sys.argv[2:] or ["k_gated_hist", "k_part_records_g", "k_seg_hist_g", "k_part<", "k_gated_reduce"]
rows = [r for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True) for r in csv.DictReader(open(f))]
by = {}
for r in rows:
    name = r["Kernel_Name"].replace("(anonymous namespace)::", "")
    if any(w in name for w in want):
        by.setdefault(name.split("(")[0], []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for name, v in sorted(by.items()):
    print(f"{name} | {len(v)} calls, mean {sum(v) / len(v):.1f}, {min(v):.1f}-{max(v):.1f} us")
print(f"all kernels of the process: {sum(int(r['End_Timestamp']) - int(r['Start_Timestamp']) for r in rows) / 1e6:.3f} ms in {len(rows)} dispatches")

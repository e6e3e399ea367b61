"""Diagnostic: per kernel and launch shape, the spread of the durations in a rocprofv3 --kernel-trace CSV (us).
usage: tools/trace_kernel_stats.py <dir or kernel_trace.csv> [substring ...]   -- only kernels whose name holds one of the substrings"""
import csv, glob, os, sys
import numpy as np

src = sys.argv[1]
if os.path.isdir(src):
    src = sorted(glob.glob(os.path.join(src, "**", "*kernel_trace.csv"), recursive=True))[0]
want = sys.argv[2:]
rows = {}
with open(src, newline="") as f:
    for r in csv.DictReader(f):
        name = r["Kernel_Name"].split("(")[0]
        if want and not any(w in name for w in want):
            continue
        shape = "%sx%s/%s" % (r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"])
        rows.setdefault((name, shape), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
for (name, shape), d in sorted(rows.items()):
    d = np.array(d)
    print("%-60s %-18s n %5d  min %7.2f  p10 %7.2f  median %7.2f  mean %7.2f  p90 %7.2f"
          % (name[-60:], shape, len(d), d.min(), np.percentile(d, 10), np.median(d), d.mean(), np.percentile(d, 90)))

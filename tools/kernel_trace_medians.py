#!/usr/bin/env python3
"""Per-kernel medians from a rocprofv3 kernel trace (its --stats table holds only mean, min and max, and under the profiler single
launches of 10 ... 30 us pull the mean of a 5 us kernel about).  The three kernels with the largest total duration, per launch in us.
    rocprofv3 -f csv --kernel-trace --stats -d DIR/trace -o trace -- python bench.py --steps 20 --warmup 5 --no-extras --no-cpu-baseline
    python tools/kernel_trace_medians.py <label> DIR/trace
profiles/r10a/kernel_trace_medians.txt is four such runs (parent, new, parent, new on one box)."""
import csv
import glob
import sys

import numpy as np

label, d = sys.argv[1], sys.argv[2]
f = glob.glob(d + "/**/*kernel_trace.csv", recursive=True)[0]
by = {}
for r in csv.DictReader(open(f)):
    by.setdefault(r["Kernel_Name"], []).append(int(r["End_Timestamp"]) - int(r["Start_Timestamp"]))
for k, v in sorted(by.items(), key=lambda kv: -sum(kv[1]))[:3]:
    v = np.array(v)
    print(f"{label}: {k[:60]:60s} calls {len(v):5d}  median {np.median(v)/1e3:.2f}  mean {v.mean()/1e3:.2f}  p10 {np.percentile(v,10)/1e3:.2f}  "
          f"p90 {np.percentile(v,90)/1e3:.2f}  min {v.min()/1e3:.2f}  max {v.max()/1e3:.2f} us", flush=True)

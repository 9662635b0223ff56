#!/usr/bin/env python3
"""T(B), T(2B) and the fixed per-launch part f = 2 T(B) - T(2B) of the three conv2 kernels from a rocprofv3 kernel trace
of bench.py (each runs once at 2B in the discriminator step and once at B in the generator half of every iteration):
tools/trace_fixed_cost.py <rocprofv3 output directory>.  Launches are taken in start order, the first quarter is dropped, and the two
alternating classes are told apart by their medians.  Use a trace of `bench.py --no-graph --no-overlap` for kernel times
that other kernels do not stretch."""
import collections
import csv
import glob
import statistics as st
import sys

KERNELS = ("conv2_fwd_kernel", "conv2_bwd_weight_kernel", "conv2_bwd_data_kernel")
f = glob.glob(sys.argv[1] + "/*/*_kernel_trace.csv")[0]
d = collections.defaultdict(list)
for r in csv.DictReader(open(f)):
    for n in KERNELS:
        if n in r["Kernel_Name"]:
            d[n].append((int(r["Start_Timestamp"]), (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3))
for n, v in d.items():
    v.sort()
    x = [dur for _, dur in v][len(v) // 4:]
    a, b = x[0::2], x[1::2]
    if st.median(a) < st.median(b):
        a, b = b, a
    q = lambda s, p: sorted(s)[int(p * (len(s) - 1))]  # noqa: E731
    print(f"{n:26s} n={len(x)} T(2B) med {st.median(a):6.2f} [p10 {q(a, .1):6.2f} p90 {q(a, .9):6.2f}]  "
          f"T(B) med {st.median(b):6.2f} [p10 {q(b, .1):6.2f} p90 {q(b, .9):6.2f}]  f={2 * st.median(b) - st.median(a):5.2f}")

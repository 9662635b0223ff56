#!/usr/bin/env python3
"""T(2B) and T(B) of every gemm_bf16_fast instance from a rocprofv3 kernel trace of bench.py (fc1's three products run
once at 2B in the discriminator step and once at B in the generator half of every iteration):
tools/trace_gemm_split.py <rocprofv3 output directory> [kernel name substring, default gemm_bf16_fast].
Reads the trace as CSV (*_kernel_trace.csv) or as the profiler's database (*_results.db), whichever the run wrote.
The method of tools/trace_fixed_cost.py: launches of one (instance, grid) in start order, the first quarter dropped;
where an instance runs with one grid at both batch sizes (fc1 dW) the two alternating classes are told apart by their
medians.  Use a trace of `bench.py --no-graph --no-overlap` for kernel times that other kernels do not stretch."""
import collections
import csv
import glob
import sqlite3
import statistics as st
import sys


def launches(directory):
    """(kernel name, workgroups, start ns, end ns) of every dispatch"""
    files = glob.glob(directory + "/*/*_kernel_trace.csv")
    if files:
        for r in csv.DictReader(open(files[0])):
            yield (r["Kernel_Name"], int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"])),
                   int(r["Start_Timestamp"]), int(r["End_Timestamp"]))
        return
    db = sqlite3.connect(glob.glob(directory + "/*/*_results.db")[0])
    for name, grid, wg, start, end in db.execute('select name, grid_x, workgroup_x, start, "end" from kernels'):
        yield name, grid // max(1, wg), start, end


want = sys.argv[2] if len(sys.argv) > 2 else "gemm_bf16_fast"
d = collections.defaultdict(list)
for name, wgs, start, end in launches(sys.argv[1]):
    if want in name:
        name = name.replace("(anonymous namespace)::", "").replace("void ", "").replace("(GemmArgs)", "")
        d[(name, wgs)].append((start, (end - start) / 1e3))
q = lambda s, p: sorted(s)[int(p * (len(s) - 1))]  # noqa: E731
for (name, wgs), v in sorted(d.items()):
    v.sort()
    x = [dur for _, dur in v][len(v) // 4:]
    if len(x) < 8:
        continue
    a, b = x[0::2], x[1::2]
    if st.median(a) < st.median(b):
        a, b = b, a
    if st.median(a) < 1.08 * st.median(b):      # one class
        print(f"{name:58s} wgs={wgs:5d} n={len(x):3d} med {st.median(x):6.2f} [p10 {q(x, .1):6.2f} p90 {q(x, .9):6.2f}]")
    else:
        print(f"{name:58s} wgs={wgs:5d} n={len(x):3d} long med {st.median(a):6.2f} [p10 {q(a, .1):6.2f} p90 {q(a, .9):6.2f}]"
              f"  short med {st.median(b):6.2f} [p10 {q(b, .1):6.2f} p90 {q(b, .9):6.2f}]")

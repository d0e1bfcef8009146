#!/usr/bin/env python3
"""conv_cb -> cb_reduce_* pairs out of a rocprofv3 kernel trace:  python tools/cb_gap_table.py <..._kernel_trace.csv> [label]
    rocprofv3 --kernel-trace --stats -- python bench.py --steps 20 --warmup 5 --full --no-cpu-baseline --no-extra
A slab launch leaves its fp32 partials dirty in the L2s and the reducer behind it reads them on other XCDs: the write-back may sit in the
GAP between the two dispatches and in neither duration, so per-kernel averages cannot show a change of the store policy.  Per queue the
dispatches are ordered by start; every slab-writing conv_cb (epilogue 0: last template argument) whose successor on the queue is a reducer
makes a pair.  Pairs are grouped by the conv_cb grid (workgroups x, y: the depth at the benchmark shape) and the reducer; printed are the
medians (and 10th / 90th percentiles of the gap) in microseconds:
    conv = conv_cb duration, gap = reducer start - conv_cb end, red = reducer duration, span = conv_cb start -> reducer end."""
import csv
import re
import statistics
import sys
from collections import defaultdict

path = sys.argv[1]
label = sys.argv[2] if len(sys.argv) > 2 else path
rows = defaultdict(list)
with open(path, newline="") as f:
    for r in csv.DictReader(f):
        rows[(r.get("Agent_Id"), r.get("Queue_Id"))].append(
            (int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"], int(r["Grid_Size_X"]) // max(int(r["Workgroup_Size_X"]), 1),
             int(r["Grid_Size_Y"]) // max(int(r["Workgroup_Size_Y"]), 1)))


def slab_conv(name):
    if "conv_cb_x3_kernel" in name:
        return True
    m = re.search(r"conv_cb_kernel<[^()]*?(\d)>\(", name) or re.search(r"conv_cb_kernelI\w*?Li(\d)EEEv", name)   # demangled or mangled name
    return bool(m) and m.group(1) == "0"


pairs = defaultdict(list)
for q in rows.values():
    q.sort()
    for (s0, e0, n0, gx, gy), (s1, e1, n1, _, _) in zip(q, q[1:]):
        if slab_conv(n0) and "cb_reduce_" in n1:
            red = "gn" if "cb_reduce_gn" in n1 else "ln"
            pairs[(gx, gy, red)].append((e0 - s0, s1 - e0, e1 - s1, e1 - s0))

print(f"# {label}: conv_cb -> cb_reduce pairs (medians, us; gap also p10 / p90)")
print(f"# {'grid x':>6} {'y':>4} {'red':>3} {'pairs':>6} {'conv':>7} {'gap':>7} {'p10':>7} {'p90':>7} {'red':>7} {'span':>7}")
tot = [0.0, 0.0, 0.0, 0.0]
n_all = 0
for key in sorted(pairs):
    v = pairs[key]
    med = [statistics.median(c) / 1e3 for c in zip(*v)]
    gaps = sorted(p[1] / 1e3 for p in v)
    p10, p90 = gaps[len(gaps) // 10], gaps[(len(gaps) * 9) // 10]
    print(f"  {key[0]:6d} {key[1]:4d} {key[2]:>3} {len(v):6d} {med[0]:7.2f} {med[1]:7.2f} {p10:7.2f} {p90:7.2f} {med[2]:7.2f} {med[3]:7.2f}")
    for i in range(4):
        tot[i] += sum(p[i] for p in v) / 1e3
    n_all += len(v)
if n_all:
    print(f"  all pairs: {n_all}, mean per pair  conv {tot[0] / n_all:.2f}  gap {tot[1] / n_all:.2f}  red {tot[2] / n_all:.2f}  span {tot[3] / n_all:.2f} us")

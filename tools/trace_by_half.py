#!/usr/bin/env python3
"""Kernel durations and launch grids by half of the solve, from a rocprofv3 --kernel-trace CSV of a small-model iLQR run:
tools/trace_by_half.py <kernel_trace.csv> [steps per solve, default 301].  Per hardware queue in dispatch order a k_solve_init starts a
solve; launch i of a kernel inside it is batch step i (launches past the last step are the empty ones the host enqueued before it saw
the batch finished).  Prints, for the scan kernel and k_forward2: launches, mean / p90 duration (us) and mean workgroups per launch
for the first half, the second half and all steps."""
import csv, sys
from collections import defaultdict

rows = list(csv.DictReader(open(sys.argv[1])))
steps = int(sys.argv[2]) if len(sys.argv) > 2 else 301
half = steps // 2
rows.sort(key=lambda r: int(r["Start_Timestamp"]))
kinds = {"k_expand_backward_scan": "scan", "k_forward2": "k_forward2"}
step = defaultdict(lambda: defaultdict(int))  # queue -> kind -> next step
dur = defaultdict(list)
grid = defaultdict(list)
for r in rows:
    q = r.get("Queue_Id", "0")
    name = r["Kernel_Name"]
    if "k_solve_init" in name:
        step[q].clear()
        continue
    for sub, kind in kinds.items():
        if sub in name:
            i = step[q][kind]
            step[q][kind] += 1
            if i >= steps:
                break
            us = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
            wgs = int(r["Grid_Size_X"]) // max(1, int(r["Workgroup_Size_X"]))
            for part in ("first" if i < half else "last", "all"):
                dur[kind, part].append(us)
                grid[kind, part].append(wgs)
            break
for kind in kinds.values():
    for part in ("first", "last", "all"):
        d = sorted(dur[kind, part])
        if not d:
            continue
        g = grid[kind, part]
        print(f"{kind:12s} {part:5s} launches {len(d):6d}  mean {sum(d) / len(d):7.1f} us  p90 {d[int(0.9 * (len(d) - 1))]:7.1f} us  "
              f"workgroups per launch {sum(g) / len(g):7.1f}  (total {sum(g)})")

#!/usr/bin/env python3
"""Per-step summary of a rocprofv3 kernel_trace.csv with the launches grouped by (kernel name, grid, workgroup size), for kernels whose name
alone does not say which layer ran them (MIOpen / rocBLAS kernels): python tools/kgroups.py kernel_trace.csv n_steps [name regex]"""
import csv, re, sys
from collections import defaultdict
rows = csv.DictReader(open(sys.argv[1]))
steps = float(sys.argv[2])
pat = re.compile(sys.argv[3], re.I) if len(sys.argv) > 3 else None
g = defaultdict(lambda: [0, 0.0, 0.0])
for r in rows:
    name = r.get("Kernel_Name", "")
    if pat and not pat.search(name):
        continue
    d = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3
    k = (name[:150], r.get("Grid_Size_X") or r.get("Grid_Size"), r.get("Grid_Size_Y"), r.get("Workgroup_Size_X") or r.get("Workgroup_Size"))
    e = g[k]
    e[0] += 1; e[1] += d; e[2] = max(e[2], d)
tot = sum(e[1] for e in g.values())
print(f"total {tot / 1e3 / steps:.3f} ms/step in {sum(e[0] for e in g.values()) / steps:.1f} launches/step")
for k, e in sorted(g.items(), key=lambda kv: -kv[1][1])[:120]:
    print(f"{e[1] / 1e3 / steps:8.3f} ms/step  launches/step {e[0] / steps:6.2f}  avg {e[1] / e[0]:8.1f} us  max {e[2]:8.1f} us  grid {k[1]}x{k[2]} wg {k[3]}  {k[0]}")

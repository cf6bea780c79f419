#!/usr/bin/env python3
"""Per-level durations of the pyramid's resize launches from rocprofv3 kernel traces.

  python tools/resize_levels.py DIR [DIR ...]      # each DIR is searched for *kernel_trace.csv (rocprofv3 --kernel-trace --output-format csv)

The resize launches of a step follow each other in the stream (levels 1, 2, ...): every run of consecutive k_resize_level / k_resize_level_rows
launches is one pyramid, the position in the run is the level.  Prints, per DIR, one JSON line: the mean duration in microseconds per level
with the kernel that ran it, and the mean sum per step.  Warm-up pyramids count like the others (same batch, same kernels).
"""
import csv
import glob
import json
import os
import sys
from collections import defaultdict


def levels_of(path):
    rows = []
    with open(path) as fh:
        for r in csv.DictReader(fh):
            name = r["Kernel_Name"].split("(")[0].split("uvo::")[-1].split("<")[0]
            rows.append((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), name))
    rows.sort()
    runs, cur = [], []
    for t0, t1, name in rows:
        if name.startswith("k_resize_level"):
            cur.append((name, (t1 - t0) / 1e3))
        elif cur:
            runs.append(cur)
            cur = []
    if cur:
        runs.append(cur)
    return runs


def main():
    for d in sys.argv[1:]:
        runs = []
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            runs += levels_of(path)
        if not runs:
            print(json.dumps({"dir": d, "error": "no resize launches"}))
            continue
        depth = max(len(r) for r in runs)
        runs = [r for r in runs if len(r) == depth]     # (a run cut by the end of the trace)
        per = defaultdict(list)
        for r in runs:
            for l, (name, us) in enumerate(r, 1):
                per[(l, name)].append(us)
        sums = sorted(sum(us for _, us in r) for r in runs)
        print(json.dumps({"dir": d, "pyramids": len(runs), "sum_us_mean": round(sum(sums) / len(sums), 2), "sum_us_median": round(sums[len(sums) // 2], 2),
                          "levels": {"%d %s" % k: round(sum(v) / len(v), 2) for k, v in sorted(per.items())}}))


if __name__ == "__main__":
    main()

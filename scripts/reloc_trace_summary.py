"""Kernel-only durations of scripts/reloc_bench.py from a rocprofv3 kernel trace:
    rocprofv3 --kernel-trace --output-format csv -d DIR -o reloc -- python scripts/reloc_bench.py
    python scripts/reloc_trace_summary.py DIR [out.csv]
One row per (kernel, grid size) of the fitness kernels: dispatches, median and total duration in microseconds.  The grid tells the
calls apart: fitness_kernel over the whole 65 536-point scan runs 256 blocks, over the 4 096-point subset 16; reloc_score_kernel runs one
block per (256-point chunk, 8 poses)."""
import csv
import glob
import os
import sys

import numpy as np

KERNELS = ("fitness_kernel", "sum_partials_kernel", "reloc_score_kernel", "reloc_reduce_kernel")


def main():
    d = sys.argv[1]
    files = glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no kernel_trace.csv under {d}")
    rows = {}
    for f in files:
        with open(f) as fh:
            for r in csv.DictReader(fh):
                name = next((k for k in KERNELS if k in r["Kernel_Name"]), None)
                if name is None:
                    continue
                grid = int(r.get("Grid_Size") or r.get("Grid_Size_X"))
                dur = (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3
                rows.setdefault((name, grid), []).append(dur)
    out = [("kernel", "grid_threads", "dispatches", "median_us", "total_us")]
    for (name, grid), v in sorted(rows.items()):
        out.append((name, grid, len(v), round(float(np.median(v)), 3), round(float(np.sum(v)), 1)))
    w = csv.writer(open(sys.argv[2], "w", newline="") if len(sys.argv) > 2 else sys.stdout)
    w.writerows(out)


if __name__ == "__main__":
    main()

"""Kernel times of `rocprofv3 --kernel-trace --stats -- python scripts/bench_mmr.py --trace` (the rocpd database it writes): every
launch of mmr_kernel with its grid (= number of pools) and of the gather kernels, median duration per (kernel, grid).

    python scripts/mmr_trace_summary.py <results.db>
"""
import sqlite3
import sys
from collections import defaultdict

import numpy as np


def main(db):
    c = sqlite3.connect(db)
    cols = [r[1] for r in c.execute("pragma table_info(kernels)")]
    grid = "grid_x" if "grid_x" in cols else ("grid_size_x" if "grid_size_x" in cols else None)
    wg = "workgroup_x" if "workgroup_x" in cols else ("workgroup_size_x" if "workgroup_size_x" in cols else None)
    q = f"select name, duration, {grid or 0}, {wg or 1} from kernels order by start"
    by = defaultdict(list)
    for name, dur, g, w in c.execute(q):
        short = name.split("(")[0]
        if "mmr_kernel" in short or "gather_dot" in short:
            by[(short, int(g) // max(int(w), 1) if grid else 0)].append(dur / 1e3)
    for (name, blocks), us in sorted(by.items()):
        print(f"{name:60s} blocks {blocks:6d}  launches {len(us):3d}  median {np.median(us):9.1f} us  min {min(us):9.1f} us")


if __name__ == "__main__":
    main(sys.argv[1])

"""Kernel times of `rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python scripts/bench_hubness.py --trace --dim D --nq Q`
(one configuration per profiler run, CALLS calls of the table build in each): per run directory the hubness kernels' launches, their
summed duration per call and the fraction of the unfused packed-f32 roof that is.

    python scripts/hubness_trace_summary.py [--calls 2] [--rows 10000000] DIR_dim384_nq1024 ...
"""
import argparse
import csv
import glob
import os
import re


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=2)
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("dirs", nargs="+")
    args = ap.parse_args()
    for d in args.dirs:
        m = re.search(r"dim(\d+)_nq(\d+)", d)
        dim, nq = (int(m.group(1)), int(m.group(2))) if m else (0, 0)
        for path in sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)):
            for row in csv.DictReader(open(path)):
                name = row["Name"].replace("(anonymous namespace)::", "").split("(")[0]
                if "hubness" not in name:
                    continue
                calls, total_ns = int(row["Calls"]), float(row["TotalDurationNs"])
                per_call_ms = total_ns / args.calls / 1e6
                line = f"dim {dim:4d} Q {nq:5d}  {name:70s} launches {calls:4d}  avg {float(row['AverageNs']) / 1e3:10.1f} us  per table {per_call_ms:9.2f} ms"
                if "hubness_kernel" in name and dim and nq:
                    tflops = 2.0 * args.rows * nq * dim / (per_call_ms * 1e-3) / 1e12
                    line += f"  {tflops:6.2f} TFLOP/s unfused = {tflops / (157.3 / 2):.3f} of the roof"
                print(line)


if __name__ == "__main__":
    main()

"""Batched search on a Quantization::F32 index: throughput, copy build time and the F16 index of the same vectors beside it.

    python scripts/bench_f32_batched.py --rows 1000000 10000000 --label this        # writes profiles/f32_batched/<label>_<rows>.json
    python scripts/bench_f32_batched.py --tree /path/to/another/checkout --label parent ...   # the same script on another build
    rocprofv3 --kernel-trace --stats -d DIR -- python scripts/bench_f32_batched.py --rows 1000000 --steps 5 --trace
    python scripts/bench_f32_batched.py --summarise-trace DIR --label this         # per-kernel totals of that run

Method: the bench's clustered corpus (fsgpu_bench_fixture_device, the reference's generator) generated in HBM as f32 rows and adopted
as an F32 index; 1,024 device-resident queries per step, k = 10; every step between two device events, warm-up 3, >= 20 timed steps,
the MEDIAN step; fallbacks summed over the timed steps (must be 0 on this corpus).  A build without fsgpu_index_create_f32_device
(the parent commit) gets the same rows through an F32 FSVI file, up to 2M rows.  A run without a GPU fails; nothing is estimated.

Roofline of the path this replaces (scan_topk_f32_kernel: four queries per pass over the f32 slab): rows x dim x 4 bytes per four
queries at the 8 TB/s HBM peak — 20.8 k queries/s at 1M x 384, 2.1 k at 10M x 384; printed next to every measurement.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTERS, NOISE = 64, 0.30
HBM_PEAK = 8.0e12


def fixture(torch, lib, check, first, n, dim, device, seed_base, as_f16):
    out = torch.empty((n, dim), dtype=torch.float16 if as_f16 else torch.float32, device=device)
    check(lib.fsgpu_bench_fixture_device(device.index or 0, first, n, dim, CLUSTERS, NOISE, seed_base, 1 if as_f16 else 0, out.data_ptr(), None))
    return out


def timed_steps(torch, be, queries, k, warmup, steps):
    for _ in range(warmup):
        be.search_batched(queries, k)
    torch.cuda.synchronize()
    ms, fallbacks = [], 0
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        be.search_batched(queries, k)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
        fallbacks += int(be.last_fallbacks)
    return ms, fallbacks


def open_f32_index(fa, torch, slab32, tmpdir):
    """An F32 index over the rows of slab32 (device tensor) -> (index, how it was made)."""
    n, dim = slab32.shape
    if hasattr(fa.VectorIndex, "from_device_slab_f32"):
        return fa.VectorIndex.from_device_slab_f32(slab32.data_ptr(), n, dim, keepalive=slab32), "fsgpu_index_create_f32_device"
    if n > 2_000_000:
        raise SystemExit("this build has no fsgpu_index_create_f32_device and the F32 FSVI detour is limited to 2M rows")
    import ctypes as C
    import numpy as np
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    host = np.ascontiguousarray(slab32.cpu().numpy(), dtype=np.float32)
    path = os.path.join(tmpdir, f"f32_{n}.fsvi")
    ids = [b"d%08d" % i for i in range(n)]          # (fa.write_fsvi's arguments, without a Python list of a million vectors)
    arr = (C.c_char_p * n)(*ids)
    lens = np.full(n, 9, dtype=np.uint32)
    check(_lib.lib().fsgpu_fsvi_write_quant(path.encode(), b"emb", b"r1", dim, n, C.cast(arr, C.c_void_p), lens.ctypes.data, host.ctypes.data,
                                            1, 0, 0))
    return fa.VectorIndex.open(path), "F32 FSVI file (rows in doc-id-hash order)"


def run(args):
    if args.tree:
        sys.path.insert(0, os.path.abspath(args.tree))
    else:
        sys.path.insert(0, ROOT)
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    from frankensearch_amd.sharded import GpuShardBackend

    lib = _lib.lib()
    if lib.fsgpu_device_count() < 1 or not torch.cuda.is_available():
        raise SystemExit("bench_f32_batched needs a GPU: nothing is estimated without one")
    dev = torch.device("cuda", 0)
    out_dir = args.out_dir or os.path.join(ROOT, "profiles", "f32_batched")
    os.makedirs(out_dir, exist_ok=True)
    for rows in args.rows:
        dim, k, nq = args.dim, args.k, args.nq
        res = {"label": args.label, "rows": rows, "dim": dim, "k": k, "queries_per_step": nq, "warmup": args.warmup, "steps": args.steps,
               "library": os.path.abspath(_lib.LIB_PATH), "device": torch.cuda.get_device_name(0),
               "old_path_roofline_qps": 4.0 * HBM_PEAK / (rows * dim * 4.0)}
        queries = fixture(torch, lib, check, 0, nq, dim, dev, 0xDEAD0000, False)
        with tempfile.TemporaryDirectory() as tmpdir:
            slab32 = fixture(torch, lib, check, 0, rows, dim, dev, 1, False)
            idx, how = open_f32_index(fa, torch, slab32, tmpdir)
            res["f32_index_from"] = how
            be = GpuShardBackend(idx, dev, batched=True)
            if not args.trace and hasattr(idx, "int8_filter_bound") and hasattr(fa.VectorIndex, "from_device_slab_f32"):
                # copy build: a fresh handle per rotation mode, host clock around a call that ends in a device synchronise
                for mode, name in ((1, "unrotated"), (2, "rotated")):
                    fresh = fa.VectorIndex.from_device_slab_f32(slab32.data_ptr(), rows, dim, keepalive=slab32)
                    fresh.set_filter_rotation(mode)
                    probe = queries[:1].cpu().numpy()
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    fresh.int8_filter_bound(probe)
                    res[f"f32_copy_build_ms_{name}"] = (time.perf_counter() - t0) * 1e3
                    t0 = time.perf_counter()
                    fresh.int8_filter_bound(probe)       # the same call with the copy in place: what of the above is not the build
                    res[f"f32_copy_build_ms_{name}"] -= (time.perf_counter() - t0) * 1e3
                    fresh.close()
            ms, fb = timed_steps(torch, be, queries, k, args.warmup, args.steps)
            med = statistics.median(ms)
            st = idx.batched_filter_stats()
            res.update({"f32_step_ms_median": med, "f32_step_ms_min": min(ms), "f32_step_ms_max": max(ms), "f32_qps": nq / (med * 1e-3),
                        "f32_fallbacks": fb, "f32_int8_queries": st["int8_queries"], "f32_filter_rotated": bool(idx.filter_rotated()),
                        "f32_main_pass_kernel": lib.fsgpu_last_main_pass_kernel().decode()})
            if not args.trace and args.checksum:
                r, s, c = be.search_batched(queries, k)
                res["f32_rows_checksum"] = int(r.to(torch.int64).sum().item())
                res["f32_score_bits_checksum"] = int(s.view(torch.int32).to(torch.int64).sum().item())
            idx.close()
            del be, idx, slab32
            torch.cuda.empty_cache()
            if args.f16:   # context: the F16 index of the same vectors (the int8 copy has the same shape; the finish reads rows half as wide)
                slab16 = fixture(torch, lib, check, 0, rows, dim, dev, 1, True)
                idx16 = fa.VectorIndex.from_device_slab(slab16.data_ptr(), rows, dim, keepalive=slab16)
                be16 = GpuShardBackend(idx16, dev, batched=True)
                ms16, fb16 = timed_steps(torch, be16, queries, k, args.warmup, args.steps)
                med16 = statistics.median(ms16)
                res.update({"f16_step_ms_median": med16, "f16_qps": nq / (med16 * 1e-3), "f16_fallbacks": fb16,
                            "f16_main_pass_kernel": lib.fsgpu_last_main_pass_kernel().decode()})
                idx16.close()
                del be16, idx16, slab16
                torch.cuda.empty_cache()
        res["above_old_path_roofline"] = bool(res["f32_qps"] > res["old_path_roofline_qps"])
        print(json.dumps(res))
        if not args.trace:
            suffix = f"_{args.run}" if args.run else ""
            with open(os.path.join(out_dir, f"{args.label}_{rows}{suffix}.json"), "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


def summarise_trace(args):
    """Per-kernel totals of a rocprofv3 --kernel-trace --stats run: the kernels of a batched step by total time."""
    files = glob.glob(os.path.join(args.summarise_trace, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_stats.csv under {args.summarise_trace}")
    rows = []
    for path in files:
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = r.get("Name") or r.get("KernelName") or ""
                total = float(r.get("TotalDurationNs") or r.get("TotalDuration") or 0)
                calls = int(float(r.get("Calls") or 0))
                rows.append({"kernel": name[:200], "calls": calls, "total_ms": total * 1e-6, "mean_us": total * 1e-3 / max(calls, 1)})
    rows.sort(key=lambda r: -r["total_ms"])
    out_dir = args.out_dir or os.path.join(ROOT, "profiles", "f32_batched")
    os.makedirs(out_dir, exist_ok=True)
    with open(os.path.join(out_dir, f"{args.label}_kernel_stats.json"), "w") as f:
        json.dump(rows[:20], f, indent=1)
        f.write("\n")
    for r in rows[:12]:
        print(f"{r['total_ms']:10.3f} ms  {r['calls']:6d} calls  {r['mean_us']:10.1f} us  {r['kernel'][:130]}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, nargs="+", default=[1_000_000])
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--label", default="this")
    ap.add_argument("--run", default="", help="suffix of the output file (alternating runs of two builds)")
    ap.add_argument("--tree", default=None, help="import frankensearch_amd from this checkout instead of the script's own")
    ap.add_argument("--out-dir", default=None)
    ap.add_argument("--f16", action="store_true", help="also the F16 index of the same vectors")
    ap.add_argument("--checksum", action="store_true", help="sums of the rows and score bits of one step (two builds must agree)")
    ap.add_argument("--trace", action="store_true", help="a short run for rocprofv3: no copy-build timing, no files")
    ap.add_argument("--summarise-trace", default=None, metavar="DIR")
    args = ap.parse_args()
    if args.steps < 20 and not args.trace:
        raise SystemExit("at least 20 timed steps")
    if args.summarise_trace:
        summarise_trace(args)
    else:
        run(args)


if __name__ == "__main__":
    main()

"""Lab timing of fsgpu_search_topk_batched_multi_filtered (filter_gather_kernels.hip, vector_index_filtered.cpp) on one
MI355X.  Corpus: the bench generator's 10M x 384 f16 slab, built in HBM and adopted; the bench generator's queries, 1,024 per call,
k = 10.  Two workloads: 64 filters that allow 1/1,000 of the rows each, and 8 filters that allow 1/100 each (random rows; query q names
filter q mod the number of filters).  In one process, in interleaved rounds:
    a) the new call;
    b) the per-query loop of fsgpu_search_topk_filtered with each query's resident filter — timed on --loop-queries queries, scaled;
    c) one fsgpu_search_topk_batched_filtered call per filter group (the queries already grouped on the host, outside the clock).
(b) and (c) exist without the new call: they are the baselines.  (a)'s rows, score bits and counts are compared with (c)'s before
anything is timed.  The gather launch alone is timed between two events (fsgpu_index_set_profiling / fsgpu_index_scan_stats) in calls
of their own and reported against the bytes it must read (sum of the groups' list lengths x dim x 2) and the HBM peak bench.py uses.
--bench-headline runs `bench.py --gpus 1` as a child process afterwards and records its JSON line (the unfiltered path, same run).
One JSON line per measurement; --out FILE appends.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLUSTERS, NOISE = 64, 0.30
HBM_PEAK_GBPS = 8000.0   # bench.py's
SPREAD = 0.04            # box-to-box spread of the README


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--loop-queries", type=int, default=32)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--workloads", default="64:1000,8:100", help="filters:divisor pairs (a filter allows rows / divisor rows)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--bench-headline", action="store_true")
    ap.add_argument("--bench-steps", type=int, default=30)
    ap.add_argument("--bench-warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, ROOT)
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, dim, k, nq = args.rows, args.dim, args.k, args.queries

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    slab = torch.empty((n, dim), dtype=torch.float16, device=dev)
    check(L.fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, 1, 1, slab.data_ptr(), None))
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    check(L.fsgpu_bench_fixture_device(0, 0, nq, dim, CLUSTERS, NOISE, 0xdead0000, 0, qdev.data_ptr(), None))
    queries = np.ascontiguousarray(qdev.cpu().numpy())
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
    rng = np.random.default_rng(7)
    fb = C.c_uint32()

    for spec in args.workloads.split(","):
        nf, div = (int(v) for v in spec.split(":"))
        per = n // div
        filters = []
        for f in range(nf):
            rows = np.unique(rng.integers(0, n, per + per // 8 + 64))
            rows = rng.permutation(rows)[:per]
            mask = np.zeros(n, dtype=bool)
            mask[rows] = True
            filters.append(idx.resident_filter(mask))
        fq = (np.arange(nq) % nf).astype(np.int32)
        handles = (C.c_void_p * nf)(*[f._h.value for f in filters])
        groups = [np.flatnonzero(fq == f) for f in range(nf)]
        grouped_q = [np.ascontiguousarray(queries[g]) for g in groups]
        out_a = (np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), np.empty(nq, np.uint32))
        out_c = (np.empty((nq, k), np.uint32), np.empty((nq, k), np.float32), np.empty(nq, np.uint32))
        r1, s1, c1 = np.empty(k, np.uint32), np.empty(k, np.float32), np.empty(1, np.uint32)

        def call_a():
            t0 = time.perf_counter()
            check(L.fsgpu_search_topk_batched_multi_filtered(idx._h, queries.ctypes.data, nq, dim, k, handles, nf, fq.ctypes.data,
                                                             out_a[0].ctypes.data, out_a[1].ctypes.data, out_a[2].ctypes.data, C.byref(fb)))
            return time.perf_counter() - t0, fb.value

        def loop_b(m):
            t0 = time.perf_counter()
            for i in range(m):
                check(L.fsgpu_search_topk_filtered(idx._h, queries[i].ctypes.data, 1, dim, k, filters[fq[i]]._h, r1.ctypes.data, s1.ctypes.data,
                                                   c1.ctypes.data))
            return time.perf_counter() - t0

        def calls_c():
            t0 = time.perf_counter()
            fbs = 0
            for f in range(nf):
                g = groups[f]
                rr, ss, cc = np.empty((g.size, k), np.uint32), np.empty((g.size, k), np.float32), np.empty(g.size, np.uint32)
                check(L.fsgpu_search_topk_batched_filtered(idx._h, grouped_q[f].ctypes.data, g.size, dim, k, filters[f]._h, rr.ctypes.data,
                                                           ss.ctypes.data, cc.ctypes.data, C.byref(fb)))
                fbs += fb.value
                out_c[0][g], out_c[1][g], out_c[2][g] = rr, ss, cc
            return time.perf_counter() - t0, fbs

        t0 = time.perf_counter()
        _, first_fb = call_a()                 # builds the row lists
        first_ms = 1e3 * (time.perf_counter() - t0)
        calls_c()                              # builds the int8 copy of the slab
        loop_b(2)
        same = bool(np.array_equal(out_a[2], out_c[2]) and np.array_equal(out_a[0], out_c[0]) and
                    np.array_equal(out_a[1].view(np.uint32), out_c[1].view(np.uint32)))
        ta, tb, tc, fba, fbc = [], [], [], [], []
        for _ in range(args.rounds):
            t, f = call_a()
            ta.append(t)
            fba.append(f)
            t, f = calls_c()
            tc.append(t)
            fbc.append(f)
            tb.append(loop_b(args.loop_queries) / args.loop_queries)
        # the gather launch alone
        idx.set_profiling(True)
        idx.scan_stats(reset=True)
        for _ in range(args.rounds):
            call_a()
        ms, launches, staged = idx.scan_stats(reset=True)
        idx.set_profiling(False)
        per_launch_ms = ms / max(launches, 1)
        roof_bytes = staged // max(launches, 1) * dim * 2
        gbps = roof_bytes / (per_launch_ms * 1e-3) / 1e9 if per_launch_ms > 0 else 0.0
        qa, qb, qc = nq / statistics.median(ta), 1.0 / statistics.median(tb), nq / statistics.median(tc)
        better = max(qb, qc)
        emit(what="search_topk_batched_multi_filtered", rows=n, dim=dim, k=k, queries=nq, filters=nf, allowed_rows_per_filter=per,
             rounds=args.rounds, answers_equal_per_group_batched_filtered=same,
             a_multi_filtered_qps_median=round(qa), a_multi_filtered_qps_best=round(nq / min(ta)), a_call_ms_median=round(1e3 * statistics.median(ta), 3),
             a_fallbacks=max(fba), a_first_call_ms=round(first_ms, 1),
             b_per_query_filtered_loop_qps_median=round(qb), b_per_query_ms_median=round(1e3 * statistics.median(tb), 4), b_timed_on=args.loop_queries,
             c_batched_filtered_per_group_qps_median=round(qc), c_calls_ms_median=round(1e3 * statistics.median(tc), 3), c_fallbacks=max(fbc),
             a_over_b=round(qa / qb, 2), a_over_c=round(qa / qc, 2),
             useful=bool(qa >= better * (1.0 - SPREAD)), useful_rule="a not slower than the better of b and c, within the 4 % box-to-box spread",
             gather_launch_ms=round(per_launch_ms, 4), gather_launches_timed=int(launches), gather_roof_bytes=int(roof_bytes),
             gather_achieved_gbps=round(gbps, 1), gather_frac_of_hbm_peak=round(gbps / HBM_PEAK_GBPS, 4), hbm_peak_gbps=HBM_PEAK_GBPS,
             multi_filter_stats=list(idx.multi_filter_stats().__dict__.values()))
        for f in filters:
            f.close()
    idx.close()
    del slab
    torch.cuda.empty_cache()
    if args.bench_headline:
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(args.bench_steps), "--warmup",
                              str(args.bench_warmup)], capture_output=True, text=True, timeout=900)
        lines = [l for l in out.stdout.splitlines() if l.startswith("{")]
        if out.returncode != 0 or not lines:
            emit(what="bench.py headline", returncode=out.returncode, stderr_tail=out.stderr[-400:])
        else:
            j = json.loads(lines[-1])
            emit(what="bench.py headline", steps=args.bench_steps, warmup=args.bench_warmup,
                 **{key: j[key] for key in ("metric", "value", "unit", "queries_per_sec", "qps", "config") if key in j})


if __name__ == "__main__":
    main()

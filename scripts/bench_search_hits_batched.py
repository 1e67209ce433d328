"""Lab timing of fsgpu_search_hits_batched (search_hits_kernels.hip, vector_index_hits.cpp) on one MI355X.
Corpus: the bench generator's 10M x 384 f16 slab, built in HBM and adopted twice — once with synthetic doc ids
(fsgpu_lab_index_attach_synthetic_doc_ids), once row-level —, the bench generator's queries, k = 30, 1,024 queries per call.
    a) queries/s of fsgpu_search_hits_batched with W = 0, 100 and 1,000 resident WAL entries (a tenth of them new versions of main rows);
    b) the per-query loop — fsgpu_search_hits query by query on the same handle — timed on --loop-queries queries and scaled;
    c) fsgpu_search_topk_batched on the row-level copy of the same slab: the ceiling.
The three are timed in interleaved rounds of one process; medians and minima are reported.  One JSON line per measurement; --out FILE
appends.
--engine: fshost_two_tier_search_many (fshost_run_load_many) over two such tiers, 10M x 256 and 10M x 384, with doc_id_mode 0 and
--engine-wal resident entries on each tier, once with the exact fast tier and once with its int8 two-pass; --tree DIR measures the
package of another checkout (the parent commit's, for the figure before this call existed) with the same script.

Kernel times proper come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d trace_hits -- python scripts/bench_search_hits_batched.py --rounds 3 --wal 1000
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

CLUSTERS, NOISE = 64, 0.30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--k", type=int, default=30)
    ap.add_argument("--queries", type=int, default=1024)
    ap.add_argument("--loop-queries", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--wal", type=int, nargs="*", default=[0, 100, 1000])
    ap.add_argument("--out", default=None)
    ap.add_argument("--engine", action="store_true")
    ap.add_argument("--engine-wal", type=int, default=1000)
    ap.add_argument("--engine-queries", type=int, default=8192)
    ap.add_argument("--tree", default=ROOT)
    ap.add_argument("--label", default="this tree")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.tree))
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, dim, k, nq = args.rows, args.dim, args.k, args.queries
    rng = np.random.default_rng(1)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    if args.engine:
        from frankensearch_amd.host import NativeTwoTierSearcher
        from frankensearch_amd.synthetic import random_bert_weights
        tiers = []
        for d in (256, 384):
            t = torch.empty((n, d), dtype=torch.float16, device=dev)
            check(L.fsgpu_bench_fixture_device(0, 0, n, d, CLUSTERS, NOISE, 1, 1, t.data_ptr(), None))
            idx = fa.VectorIndex.from_device_slab(t.data_ptr(), n, d, keepalive=t)
            check(L.fsgpu_lab_index_attach_synthetic_doc_ids(idx._h))
            if args.engine_wal:
                W = args.engine_wal
                ids = [f"doc-{int(i):09d}" if j % 10 == 0 else f"new-{j:07d}" for j, i in enumerate(rng.integers(0, n, W))]
                vec = rng.standard_normal((W, d)).astype(np.float32)
                idx.append_batch(list(zip(ids, vec / np.linalg.norm(vec, axis=1, keepdims=True))))
            tiers.append(idx)
        m2v = fa.Model2VecEmbedder(np.random.default_rng(0).standard_normal((500_353, 256)).astype(np.float32), device=0)
        bert = fa.NativeEmbedder(random_bert_weights(1, 30522, 384, 6, 1536), device=0)
        for mult in (0, 3):
            s = NativeTwoTierSearcher(tiers[0], tiers[1], m2v, bert, doc_id_mode=0, fast_tier_int8_multiplier=mult)
            for rep in range(2):     # (the first builds the quantised copies and the device tables)
                r = s.run_load_many(queries=args.engine_queries, warmup_queries=1024, k=10, fast_vocab=500_353, corpus_rows=n, chunk=1024)
            emit(what="fshost_two_tier_search_many", tree=args.label, rows=n, doc_id_mode=0, fast_tier_int8_multiplier=mult,
                 wal_entries_per_tier=tiers[0].wal_record_count(), queries=r["queries"], chunk=1024, queries_per_sec=round(r["queries_per_sec"]),
                 mean_fast_search_ms=round(r["mean_fast_search_ms"], 3), mean_quality_search_ms=round(r["mean_quality_search_ms"], 3),
                 fast_fallbacks=r["fast_fallbacks"], quality_fallbacks=r["quality_fallbacks"], device_resident_handoff=r["device_resident_handoff"],
                 error_detail=r["error_detail"] if isinstance(r["error_detail"], str) else str(r["error_detail"]))
            s.close()
        return
    slab = torch.empty((n, dim), dtype=torch.float16, device=dev)
    check(L.fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, 1, 1, slab.data_ptr(), None))
    qdev = torch.empty((nq, dim), dtype=torch.float32, device=dev)
    check(L.fsgpu_bench_fixture_device(0, 0, nq, dim, CLUSTERS, NOISE, 0xdead0000, 0, qdev.data_ptr(), None))
    queries = np.ascontiguousarray(qdev.cpu().numpy())
    row_level = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
    rows = np.empty((nq, k), np.uint32)
    scores = np.empty((nq, k), np.float32)
    counts = np.empty(nq, np.uint32)
    fb = C.c_uint32()

    def ceiling():
        t0 = time.perf_counter()
        check(L.fsgpu_search_topk_batched(row_level._h, queries.ctypes.data, nq, dim, k, None, rows.ctypes.data, scores.ctypes.data,
                                          counts.ctypes.data, C.byref(fb)))
        return time.perf_counter() - t0, fb.value

    def batched(idx):
        t0 = time.perf_counter()
        check(L.fsgpu_search_hits_batched(idx._h, queries.ctypes.data, nq, dim, k, rows.ctypes.data, scores.ctypes.data, counts.ctypes.data,
                                          C.byref(fb)))
        return time.perf_counter() - t0, fb.value

    def loop(idx, m):
        one = C.c_uint32()
        t0 = time.perf_counter()
        for i in range(m):
            check(L.fsgpu_search_hits(idx._h, queries[i].ctypes.data, dim, k, rows[i].ctypes.data, scores[i].ctypes.data, C.byref(one)))
        return time.perf_counter() - t0

    for W in args.wal:
        idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
        check(L.fsgpu_lab_index_attach_synthetic_doc_ids(idx._h))
        if W:
            ids = [f"doc-{int(i):09d}" if j % 10 == 0 else f"new-{j:07d}" for j, i in enumerate(rng.integers(0, n, W))]
            vec = rng.standard_normal((W, dim)).astype(np.float32)
            idx.append_batch(list(zip(ids, vec / np.linalg.norm(vec, axis=1, keepdims=True))))
        t0 = time.perf_counter()
        _, first_fb = batched(idx)          # builds the int8 copy and the device tables
        first_ms = 1e3 * (time.perf_counter() - t0)
        ceiling()
        loop(idx, 4)
        ta, tb, tc, fbs = [], [], [], []
        for _ in range(args.rounds):        # interleaved rounds, one process
            t, f = batched(idx)
            ta.append(t)
            fbs.append(f)
            tc.append(ceiling()[0])
            tb.append(loop(idx, args.loop_queries) / args.loop_queries)
        qa, qc, qb = nq / statistics.median(ta), nq / statistics.median(tc), 1.0 / statistics.median(tb)
        emit(what="search_hits_batched", rows=n, dim=dim, k=k, queries=nq, wal_entries=idx.wal_record_count(), rounds=args.rounds,
             a_batched_qps_median=round(qa), a_batched_qps_best=round(nq / min(ta)), a_call_ms_median=round(1e3 * statistics.median(ta), 3),
             a_fallbacks=max(fbs), first_call_ms=round(first_ms, 1),
             b_per_query_loop_qps_median=round(qb), b_per_query_ms_median=round(1e3 * statistics.median(tb), 4), b_timed_on=args.loop_queries,
             c_row_level_batched_qps_median=round(qc), c_row_level_batched_qps_best=round(nq / min(tc)),
             a_over_c=round(qa / qc, 3), a_over_b=round(qa / qb, 1))
        idx.close()
    row_level.close()


if __name__ == "__main__":
    main()

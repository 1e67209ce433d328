"""Lab timing of the graph ANN search (fsgpu_ann_*; ann_kernels.hip, ann_index.cpp) on one MI355X.
Corpus and queries: the bench generator's clustered f16 slab and f32 queries, built in HBM; graph width m = 16.  Prints one JSON line
per measurement; every time is the median of `--reps` calls after a warm-up of the same shape (host clock around blocking calls).

  graph       fsgpu_index_build_knn_graph over the whole slab, and fsgpu_ann_create (the upload of the table)
  ann         per ef: queries/s at `--nq` host queries per call, the lone query's p50, rows scored and steps per query, recall@10 mean
              and minimum against the exact batched search over the same queries, flagged queries
  certify     fsgpu_ann_certify_ef over `--calib` queries at target 0.95, alpha 0.1
  exact       the exact batched search at k = 10 over the same `--nq` queries, and the lone fsgpu_search_topk, same slab, same process

    python scripts/bench_ann.py --rows 1000000 --out profiles/ann/bench_ann.jsonl
    python scripts/bench_ann.py --rows 10000000 --out profiles/ann/bench_ann.jsonl --append
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLUSTERS, NOISE = 64, 0.30


def median_ms(fn, reps):
    fn()   # warm-up of this shape
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return 1e3 * float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--efs", default="32,64,128,256")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--calib", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--n-entry", type=int, default=1024)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def fixture(n, dim, seed_base, as_f16):
        out = torch.empty((n, dim), dtype=torch.float16 if as_f16 else torch.float32, device=dev)
        check(L.fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, seed_base, 1 if as_f16 else 0, out.data_ptr(), None))
        return out

    n, dim, m, k = args.rows, args.dim, args.m, args.k
    efs = [int(e) for e in args.efs.split(",")]
    slab = fixture(n, dim, 1, True)
    queries = fixture(args.nq, dim, 0xDEAD0000, False).cpu().numpy()
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
    idx.build_knn_graph(m, n_rows=min(1024, n))   # warm-up: builds the int8 copy, probes the shapes
    t0 = time.perf_counter()
    table = idx.build_knn_graph(m)
    t_graph = time.perf_counter() - t0
    t0 = time.perf_counter()
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(n_entry=args.n_entry))
    t_upload = time.perf_counter() - t0
    emit(what="graph", rows=n, dim=dim, m=m, build_seconds=round(t_graph, 3), sources_per_s=round(n / t_graph, 1),
         upload_seconds=round(t_upload, 4), table_mb=round(table.nbytes / 1e6, 1), n_entry=args.n_entry)

    er, _, ec, _ = idx.search_batched(queries, k)
    exact_ms = median_ms(lambda: idx.search_batched(queries, k), args.reps)
    lone_ms = median_ms(lambda: idx.search_batch(queries[:1], k), args.reps)
    emit(what="exact", rows=n, dim=dim, k=k, nq=args.nq, batched_ms=round(exact_ms, 3), batched_queries_per_s=round(args.nq / exact_ms * 1e3, 1),
         lone_topk_p50_ms=round(lone_ms, 4))
    for ef in efs:
        one_ms = median_ms(lambda: ann.search(queries[0], k, ef), args.reps)
        batch_ms = median_ms(lambda: ann.search_batched(queries, k, ef), args.reps)
        rows, _, counts, flags = ann.search_batched(queries, k, ef)
        st = ann.stats   # (of a warm call)
        recall = [len(set(rows[i, :counts[i]].tolist()) & set(er[i, :ec[i]].tolist())) / max(int(ec[i]), 1) for i in range(args.nq)]
        emit(what="ann", rows=n, dim=dim, m=m, k=k, ef=ef, nq=args.nq, batched_ms=round(batch_ms, 3),
             queries_per_s=round(args.nq / batch_ms * 1e3, 1), kernel_ms=round(st.device_ms, 3), lone_p50_ms=round(one_ms, 4),
             rows_scored_per_query=round(st.rows_scored / args.nq, 1), steps_per_query=round(st.steps / args.nq, 1),
             recall_mean=round(float(np.mean(recall)), 4), recall_min=round(float(np.min(recall)), 4), flagged=int((flags != 0).sum()),
             over_exact_batched=round(exact_ms / batch_ms, 3), lone_over_exact_lone=round(lone_ms / one_ms, 3))
    t0 = time.perf_counter()
    chosen, sweep = ann.certify_ef(queries[:args.calib], efs, k, 0.95, 0.1)
    emit(what="certify", rows=n, calibration_queries=min(args.calib, args.nq), target=0.95, alpha=0.1, chosen_ef=chosen.ef_search,
         certified_recall=chosen.certified_recall, meets_target=chosen.meets_target,
         sweep=[[c.ef_search, c.certified_recall] for c in sweep], seconds=round(time.perf_counter() - t0, 3))
    ann.close()
    idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

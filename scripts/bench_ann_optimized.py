"""Lab comparison of the graph ANN search over the exact k-NN table and over the optimised table (fsgpu_knn_graph_optimize; DESIGN
3.20) on one MI355X, both in ONE process over the same slab, queries and calibration queries.

  exact16     the parent's configuration: fsgpu_index_build_knn_graph at m = 16, searched as it is
  optimised   the m = 32 table optimised to 16 columns

  --corpus bench        the bench generator's clustered f16 slab (isotropic noise inside 64 clusters), built in HBM
  --corpus structured   the contract test's generator scaled up: `--clusters` centres inside a random 8-dimensional subspace, lifted
                        to `--dim` dimensions (tests/test_knn_optimize_contract.py), made on the host

Per ef and configuration: recall@10 mean and minimum against the exact batched search, rows scored, queries/s at `--nq` queries per
call and the lone query's p50 — medians of `--reps` calls after a warm-up, the two configurations interleaved call by call;
fsgpu_ann_certify_ef at target 0.95, alpha 0.1; the optimiser's device_ms and whole-call time beside the table builds' times.

    python scripts/bench_ann_optimized.py --rows 1000000 --out profiles/ann/bench_ann_optimized.jsonl
    python scripts/bench_ann_optimized.py --rows 10000000 --out profiles/ann/bench_ann_optimized.jsonl --append
    python scripts/bench_ann_optimized.py --corpus structured --rows 1000000 --dim 64 --out profiles/ann/bench_ann_optimized.jsonl --append
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


def interleaved_median_ms(fns, reps):
    """The median time of each fn, called in turn: a drift of the box reaches every configuration alike."""
    for fn in fns:
        fn()   # warm-up of this shape
    ts = [[] for _ in fns]
    for _ in range(reps):
        for i, fn in enumerate(fns):
            t0 = time.perf_counter()
            fn()
            ts[i].append(time.perf_counter() - t0)
    return [1e3 * float(np.median(t)) for t in ts]


def structured(rng, n, centres, basis):
    out = np.empty((n, basis.shape[1]), dtype=np.float16)
    for at in range(0, n, 1 << 18):
        m = min(1 << 18, n - at)
        low = centres[rng.integers(0, centres.shape[0], m)] + 0.3 * rng.standard_normal((m, centres.shape[1]))
        x = (low @ basis).astype(np.float32)
        out[at:at + m] = (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float16)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--corpus", choices=("bench", "structured"), default="bench")
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--clusters", type=int, default=32)
    ap.add_argument("--m", type=int, default=32)
    ap.add_argument("--degree", type=int, default=16)
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
        lines.append(json.dumps(dict(corpus=args.corpus, **kw)))
        print(lines[-1], flush=True)

    n, dim, k, d = args.rows, args.dim, args.k, args.degree
    efs = [int(e) for e in args.efs.split(",")]
    if args.corpus == "bench":
        def fixture(rows, seed_base, as_f16):
            out = torch.empty((rows, dim), dtype=torch.float16 if as_f16 else torch.float32, device=dev)
            check(L.fsgpu_bench_fixture_device(0, 0, rows, dim, CLUSTERS, NOISE, seed_base, 1 if as_f16 else 0, out.data_ptr(), None))
            return out
        slab = fixture(n, 1, True)
        queries = fixture(args.nq, 0xDEAD0000, False).cpu().numpy()
    else:
        rng = np.random.default_rng(2)
        centres = rng.standard_normal((args.clusters, 8))
        basis = rng.standard_normal((8, dim))
        slab = torch.from_numpy(structured(rng, n, centres, basis)).to(dev)
        queries = structured(rng, args.nq, centres, basis).astype(np.float32)
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
    idx.build_knn_graph(d, n_rows=min(1024, n))   # warm-up: builds the int8 copy, probes the shapes

    t0 = time.perf_counter()
    exact16 = idx.build_knn_graph(d)
    t_exact16 = time.perf_counter() - t0
    t0 = time.perf_counter()
    wide = idx.build_knn_graph(args.m)
    t_wide = time.perf_counter() - t0
    idx.optimize_knn_graph(wide[:, :d], d)   # warm-up (the kernels' code objects)
    t0 = time.perf_counter()
    optimised, ost = idx.optimize_knn_graph(wide, d, want_stats=True)
    t_opt = time.perf_counter() - t0
    emit(what="tables", rows=n, dim=dim, m=args.m, degree=d, build_exact_seconds=round(t_exact16, 3), build_wide_seconds=round(t_wide, 3),
         optimize_seconds=round(t_opt, 3), optimize_device_ms=round(ost["device_ms"], 3),
         table_bytes_each_way=[int(wide.nbytes), int(optimised.nbytes)], **{key: int(v) for key, v in ost.items() if key not in ("device_ms", "rows")})

    cfg = fa.AnnConfig(n_entry=args.n_entry)
    anns = {"exact16": fa.AnnIndex(idx, exact16, cfg), "optimised": fa.AnnIndex(idx, optimised, cfg)}
    er, _, ec, _ = idx.search_batched(queries, k)
    exact_ms, lone_ms = interleaved_median_ms([lambda: idx.search_batched(queries, k), lambda: idx.search_batch(queries[:1], k)], args.reps)
    emit(what="exact", rows=n, dim=dim, k=k, nq=args.nq, batched_ms=round(exact_ms, 3), batched_queries_per_s=round(args.nq / exact_ms * 1e3, 1),
         lone_topk_p50_ms=round(lone_ms, 4))
    names = list(anns)
    for ef in efs:
        batch = interleaved_median_ms([lambda a=anns[nm]: a.search_batched(queries, k, ef) for nm in names], args.reps)
        lone = interleaved_median_ms([lambda a=anns[nm]: a.search(queries[0], k, ef) for nm in names], args.reps)
        for i, nm in enumerate(names):
            rows, _, counts, flags = anns[nm].search_batched(queries, k, ef)
            st = anns[nm].stats
            recall = [len(set(rows[q, :counts[q]].tolist()) & set(er[q, :ec[q]].tolist())) / max(int(ec[q]), 1) for q in range(args.nq)]
            emit(what="ann", table=nm, rows=n, dim=dim, k=k, ef=ef, nq=args.nq, batched_ms=round(batch[i], 3),
                 queries_per_s=round(args.nq / batch[i] * 1e3, 1), lone_p50_ms=round(lone[i], 4),
                 rows_scored_per_query=round(st.rows_scored / args.nq, 1), steps_per_query=round(st.steps / args.nq, 1),
                 recall_mean=round(float(np.mean(recall)), 4), recall_min=round(float(np.min(recall)), 4), flagged=int((flags != 0).sum()),
                 over_exact_batched=round(exact_ms / batch[i], 3))
    for nm in names:
        t0 = time.perf_counter()
        chosen, sweep = anns[nm].certify_ef(queries[:args.calib], efs, k, 0.95, 0.1)
        emit(what="certify", table=nm, rows=n, calibration_queries=min(args.calib, args.nq), target=0.95, alpha=0.1,
             chosen_ef=chosen.ef_search, certified_recall=chosen.certified_recall, meets_target=chosen.meets_target,
             sweep=[[c.ef_search, c.certified_recall] for c in sweep], seconds=round(time.perf_counter() - t0, 3))
    for a in anns.values():
        a.close()
    idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

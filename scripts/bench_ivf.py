"""Lab timing of the IVF index (fsgpu_ivf_*; ivf_kernels.hip, ivf_index.cpp) on one MI355X.  Prints one JSON line per measurement.

  --corpus bench        the bench generator's clustered f16 slab and f32 queries, built in HBM
  --corpus structured   `--clusters` centres inside a random 8-dimensional subspace, lifted to `--dim` dimensions (the corpus of
                        scripts/bench_ann_optimized.py), made on the host

  build      fsgpu_ivf_create: the whole call, and the device time per stage and per iteration (fsgpu_ivf_build_stats)
  certify    fsgpu_ivf_certify_nprobe over `--calib` queries at target 0.95, alpha 0.1
  ivf        per nprobe (and the certified one): queries/s at `--nq` host queries per call, the lone query's p50, rows scored per
             query, recall@10 mean and minimum against the exact batched search over the same queries, flagged queries
  exact      the exact batched search at k = 10 over the same `--nq` queries, and the lone fsgpu_search_topk, same slab, same process
Every time is the median of `--reps` calls after a warm-up of the same shape, one process, the measured calls of a round interleaved
(host clock around blocking calls).

    python scripts/bench_ivf.py --rows 1000000 --out profiles/ivf/bench_ivf.jsonl
    python scripts/bench_ivf.py --rows 10000000 --nlist 4096 --out profiles/ivf/bench_ivf.jsonl --append
    python scripts/bench_ivf.py --corpus structured --rows 1000000 --dim 64 --out profiles/ivf/bench_ivf.jsonl --append
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
    for fn in fns:
        fn()   # warm-up of each shape
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
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--n-train", type=int, default=0)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nprobes", default="1,4,16,64")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--calib", type=int, default=200)
    ap.add_argument("--reps", type=int, default=20)
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

    n, dim, k, nlist = args.rows, args.dim, args.k, args.nlist
    nprobes = [int(p) for p in args.nprobes.split(",") if int(p) <= min(nlist, 256)]
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
    er, _, ec, _ = idx.search_batched(queries, k)   # (builds the int8 copy, probes the shapes)

    idx.build_ivf(min(nlist, 64), iters=1, n_train=min(n, 65536)).close()   # warm-up: the kernels' code objects
    t0 = time.perf_counter()
    ivf = idx.build_ivf(nlist, iters=args.iters, n_train=args.n_train)
    t_build = time.perf_counter() - t0
    b = ivf.build_stats
    passes = b.iterations + 1   # the iterations' assignments and the final one over all live rows
    flop = 2.0 * dim * nlist * (b.rows_trained * b.iterations + n)
    emit(what="build", rows=n, dim=dim, nlist=nlist, iters=b.iterations, rows_trained=b.rows_trained, seconds=round(t_build, 3),
         assign_ms=round(b.assign_ms, 3), assign_ms_per_pass=round(b.assign_ms / passes, 3),
         assign_tflops=round(flop / (b.assign_ms * 1e-3) / 1e12, 2) if b.assign_ms else None,
         update_ms=round(b.update_ms, 3), update_ms_per_iter=round(b.update_ms / max(b.iterations, 1), 3), lists_ms=round(b.lists_ms, 3),
         lists_ms_per_pass=round(b.lists_ms / passes, 3), rows_changed_last=b.rows_changed_last, empty_lists=b.empty_lists,
         largest_list=b.largest_list, smallest_list=b.smallest_list,
         index_mb=round((n * 4 + (nlist + 1) * 8 + nlist * dim * 4) / 1e6, 1))

    t0 = time.perf_counter()
    chosen, sweep = ivf.certify_nprobe(queries[:args.calib], sorted(set(nprobes + [2, 8, 32, 128, 256]) & set(range(1, min(nlist, 256) + 1))),
                                       k, 0.95, 0.1)
    emit(what="certify", rows=n, nlist=nlist, calibration_queries=min(args.calib, args.nq), target=0.95, alpha=0.1, chosen_nprobe=chosen.ef_search,
         certified_recall=chosen.certified_recall, meets_target=chosen.meets_target,
         sweep=[[c.ef_search, c.certified_recall] for c in sweep], seconds=round(time.perf_counter() - t0, 3))
    if chosen.meets_target and chosen.ef_search not in nprobes:
        nprobes.append(chosen.ef_search)

    for p in nprobes:
        batch_ms, exact_ms, one_ms, lone_ms = interleaved_median_ms(
            [lambda: ivf.search_batched(queries, k, p), lambda: idx.search_batched(queries, k), lambda: ivf.search(queries[0], k, p),
             lambda: idx.search_batch(queries[:1], k)], args.reps)
        ivf.search(queries[0], k, p)
        lone_st = ivf.stats
        rows, _, counts, flags = ivf.search_batched(queries, k, p)
        st = ivf.stats   # (of a warm call)
        recall = [len(set(rows[i, :counts[i]].tolist()) & set(er[i, :ec[i]].tolist())) / max(int(ec[i]), 1) for i in range(args.nq)]
        emit(what="ivf", rows=n, dim=dim, nlist=nlist, k=k, nprobe=p, certified=bool(chosen.meets_target and p == chosen.ef_search), nq=args.nq,
             batched_ms=round(batch_ms, 3), queries_per_s=round(args.nq / batch_ms * 1e3, 1), device_ms=round(st.device_ms, 3),
             lone_p50_ms=round(one_ms, 4), lone_device_ms=round(lone_st.device_ms, 4), rows_scored_per_query=round(st.rows_scored / args.nq, 1),
             share_of_rows_scored=round(st.rows_scored / args.nq / n, 5), recall_mean=round(float(np.mean(recall)), 4),
             recall_min=round(float(np.min(recall)), 4), flagged=int((flags != 0).sum()), exact_batched_ms=round(exact_ms, 3),
             exact_lone_p50_ms=round(lone_ms, 4), over_exact_batched=round(exact_ms / batch_ms, 3), lone_over_exact_lone=round(lone_ms / one_ms, 3))
    ivf.close()
    idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

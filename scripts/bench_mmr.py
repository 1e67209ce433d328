"""Lab timing of MMR over index rows (fsgpu_index_mmr_rerank / _batched, mmr_kernels.hip) on one MI355X, against the host restatement
(fsgpu_mmr_rerank on vectors already in host memory, 16 threads) and against the gather alone (fsgpu_gather_dot over the same rows).
Corpus: the bench generator's 10M x 384 f16 slab, built in HBM; pools: the top-30 answers of 1,024 of its queries, so the gather is as
scattered as in use.  Every call is warmed up, then timed with a host clock around the blocking C call.  Prints one JSON line per
measurement; `--trace` runs each device call a few times only (for a rocprofv3 --kernel-trace --stats run of its own: kernel times
come from there, scripts/mmr_trace_summary.py).

    python scripts/bench_mmr.py [--rows 10000000] [--reps 20] [--trace] [--out profiles/mmr/bench_mmr.jsonl]
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLUSTERS, NOISE, DIM, POOL = 64, 0.30, 384, 30


def p50_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 4), round(1e3 * min(ts), 4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    dev = torch.device("cuda:0")

    def fixture(n, seed_base, as_f16):
        out = torch.empty((n, DIM), dtype=torch.float16 if as_f16 else torch.float32, device=dev)
        check(_lib.lib().fsgpu_bench_fixture_device(0, 0, n, DIM, CLUSTERS, NOISE, seed_base, 1 if as_f16 else 0, out.data_ptr(), None))
        return out
    slab = fixture(args.rows, 1, True)
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), args.rows, DIM, keepalive=slab)
    nq = 1024
    queries = fixture(nq, 0xDEAD0000, False).cpu().numpy()
    rows, scores, counts, _ = idx.search_batched(queries, POOL)
    assert int(counts.min()) == POOL
    rows = np.ascontiguousarray(rows, dtype=np.uint32)
    scores64 = np.ascontiguousarray(scores, dtype=np.float64)
    cfg = fa.MmrConfig(True, 0.7, POOL)
    reps = 3 if args.trace else args.reps
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    for pools in (1, 64, 256, 1024):
        r, s = rows[:pools].reshape(-1), scores64[:pools].reshape(-1)
        offs = (np.arange(pools + 1) * POOL).astype(np.uint32)
        call = (lambda: idx.mmr_rerank(r, s, POOL, cfg)) if pools == 1 else (lambda: idx.mmr_rerank_batched(r, s, offs, POOL, cfg))
        for _ in range(3):
            got = call()
        p50, mn = p50_ms(call, reps)
        orders = [got] if pools == 1 else got
        moved = sum(o.tolist() != list(range(POOL)) for o in orders)
        emit(what="device_call", pools=pools, pool=POOL, dim=DIM, rows=args.rows, reps=reps, ms_p50=p50, ms_min=mn, pools_reordered=moved)
        # the gather alone over the same rows: one dot per row against the pool's query (fsgpu_quality_scores_for_hits' kernel)
        if pools == 1:
            gather = lambda: idx.gather_dot(queries[0], r)
            for _ in range(3):
                gather()
            p50, mn = p50_ms(gather, reps)
            emit(what="gather_dot_call", pools=1, ms_p50=p50, ms_min=mn)
        if args.trace:
            continue
        # the host restatement on vectors already in host memory, 16 threads (ctypes releases the GIL around the C call)
        host_vecs = slab[torch.from_numpy(r.astype(np.int64)).to(dev)].float().cpu().numpy().reshape(pools, POOL, DIM)

        def host_one(q):
            return fa.mmr_rerank(scores64[q], host_vecs[q], POOL, cfg)
        with ThreadPoolExecutor(max_workers=16) as ex:
            host = list(ex.map(host_one, range(pools)))
            p50, mn = p50_ms(lambda: list(ex.map(host_one, range(pools))), max(3, reps // 4))
        assert all(h.tolist() == o.tolist() for h, o in zip(host, orders)), "device and host orders differ"
        emit(what="host_restatement_16_threads", pools=pools, ms_p50=p50, ms_min=mn, note="vectors already in host memory; python dispatch included")
    if not args.trace:
        # the multi-query gather (gather_dot_mq_kernel) over all 1,024 x 30 rows, through the two-tier re-scoring call that launches it
        from frankensearch_amd.two_tier import TwoTierIndex
        pair = TwoTierIndex(idx, idx)
        hits = [[("", float(scores[q, i]), int(rows[q, i])) for i in range(POOL)] for q in range(nq)]
        for _ in range(2):
            pair.quality_scores_for_hits_batched(queries, hits)
        p50, mn = p50_ms(lambda: pair.quality_scores_for_hits_batched(queries, hits), 5)
        emit(what="gather_dot_mq_call", pools=nq, ms_p50=p50, ms_min=mn, note="python packing of 30,720 hits included; kernel time: the trace")
    else:
        from frankensearch_amd.two_tier import TwoTierIndex
        pair = TwoTierIndex(idx, idx)
        hits = [[("", float(scores[q, i]), int(rows[q, i])) for i in range(POOL)] for q in range(nq)]
        for _ in range(3):
            pair.quality_scores_for_hits_batched(queries, hits)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

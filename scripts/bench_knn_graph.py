"""Lab timing of the k-NN graph build (fsgpu_index_build_knn_graph; knn_graph_kernels.hip, vector_index_knn.cpp) on one MI355X.
Corpus: the bench generator's f16 slab, built in HBM; m = 10.  Prints one JSON line per measurement.

  build       source rows per second of the device call over `--sources` rows starting at `--first` (0 = the whole graph), with the
              step's fallback and re-filter counts (corpus points as queries are a query distribution bench.py never ran)
  yardstick   the device-resident batched search at k = m + 1 over THE SAME sources as queries (rows widened on the device), the
              begin / end loop of frankensearch_amd/sharded.py with two searches in flight: the same kernel without staging, emit
              and the copy out
  host        the CPU oracle's exact search (16 threads) for a few of the sources, SCALED linearly to the source count
  searcher    fshost_two_tier_search_many over 1,024 queries with and without a graph attached, same run

    python scripts/bench_knn_graph.py --rows 1000000 --out profiles/knn_graph/bench_knn_graph.jsonl
    python scripts/bench_knn_graph.py --rows 10000000 --first 5000000 --sources 102400 --out ... --append
    python scripts/bench_knn_graph.py --only-searcher --rows 1000000 --out ... --append
    rocprofv3 --kernel-trace --stats --output-format csv -d trace_knn -- python scripts/bench_knn_graph.py --trace --rows 1000000 --sources 102400

On a shared card every step gets a process and a time limit of its own, chained so that a step that fails ends the series.
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CLUSTERS, NOISE, CHUNK = 64, 0.30, 1024


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--m", type=int, default=10)
    ap.add_argument("--first", type=int, default=0)
    ap.add_argument("--sources", type=int, default=0)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--host-sources", type=int, default=32)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--only-searcher", action="store_true")
    ap.add_argument("--no-searcher", action="store_true")
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

    m, k = args.m, args.m + 1
    if not args.only_searcher:
        n, dim = args.rows, args.dim
        nsrc = args.sources or n
        slab = fixture(n, dim, 1, True)
        idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
        idx.build_knn_graph(m, first_row=args.first, n_rows=min(CHUNK, nsrc))     # warm-up: builds the int8 copy, probes the shapes
        best, rows = None, None
        for _ in range(1 if args.trace else args.reps):
            f0 = idx.batched_filter_stats()
            t0 = time.perf_counter()
            rows = idx.build_knn_graph(m, first_row=args.first, n_rows=nsrc)
            dt = time.perf_counter() - t0
            f1 = idx.batched_filter_stats()
            st = (C.c_uint64 * 4)()
            check(L.fsgpu_lab_index_knn_build_stats(idx._h, st))
            rec = dict(what="build", rows=n, dim=dim, m=m, first=args.first, sources=nsrc, seconds=round(dt, 4),
                       sources_per_s=round(nsrc / dt, 1), steps=int(st[0]), fallbacks=int(st[2]), late_answers=int(st[3]),
                       int8_filtered=f1["int8_queries"] - f0["int8_queries"], refiltered_f16=f1["refiltered_f16"] - f0["refiltered_f16"],
                       whole_graph_seconds_scaled=round(dt * n / nsrc, 2), scaled=nsrc != n,
                       pad_entries=int((rows == 0xFFFFFFFF).sum()))
            if best is None or rec["seconds"] < best["seconds"]:
                best = rec
        emit(**best)
        if not args.trace:
            # the yardstick: the same sources as device-resident queries through the begin / end loop, two searches in flight
            def yardstick():
                outs = [tuple(torch.empty((CHUNK, k), dtype=t, device=dev) for t in (torch.int32, torch.float32)) +
                        (torch.empty((CHUNK,), dtype=torch.int32, device=dev),) for _ in range(2)]
                stream = torch.cuda.current_stream(dev).cuda_stream
                pending, fb_total, late_total = [], 0, 0

                def end(t):
                    fb, late = C.c_uint32(), C.c_uint32()
                    check(L.fsgpu_search_topk_batched_device_end_late(idx._h, t, C.byref(fb), C.byref(late)))
                    return fb.value, late.value
                for c, lo in enumerate(range(args.first, args.first + nsrc, CHUNK)):
                    b = min(CHUNK, args.first + nsrc - lo)
                    if len(pending) == 2:
                        fb, late = end(pending.pop(0)[0])
                        fb_total, late_total = fb_total + fb, late_total + late
                    q = slab[lo:lo + b].float().contiguous()
                    r_, s_, c_ = outs[c & 1]
                    ticket = C.c_int32(-1)
                    check(L.fsgpu_search_topk_batched_device_begin(idx._h, q.data_ptr(), b, dim, k, None, r_.data_ptr(), s_.data_ptr(),
                                                                   c_.data_ptr(), None, stream, C.byref(ticket)))
                    pending.append((ticket.value, q))
                for t, _ in pending:
                    fb, late = end(t)
                    fb_total, late_total = fb_total + fb, late_total + late
                torch.cuda.synchronize(dev)
                return fb_total, late_total
            yardstick_first = min(CHUNK * 2, nsrc)
            ybest = None
            for _ in range(args.reps):
                t0 = time.perf_counter()
                fb, late = yardstick()
                dt = time.perf_counter() - t0
                if ybest is None or dt < ybest[0]:
                    ybest = (dt, fb, late)
            emit(what="yardstick_batched_search_k11", rows=n, dim=dim, k=k, queries=nsrc, seconds=round(ybest[0], 4),
                 queries_per_s=round(nsrc / ybest[0], 1), fallbacks=ybest[1], late_answers=ybest[2],
                 build_over_yardstick=round((nsrc / best["seconds"]) / (nsrc / ybest[0]), 3), warmup_queries=yardstick_first)
            # the host: the CPU oracle's exact search, 16 threads, on a few sources; scaled linearly in the number of sources
            from oracle import oracle
            oracle.build()
            hs = min(args.host_sources, nsrc)
            host_slab = slab.cpu().numpy().view(np.uint16)
            picks = np.linspace(args.first, args.first + nsrc - 1, hs).astype(np.int64)
            wide = slab[torch.as_tensor(picks, device=dev)].float().cpu().numpy()
            t0 = time.perf_counter()
            same = True
            for i, s in enumerate(picks):
                r, _ = oracle.search_top_k(host_slab, wide[i], k, nthreads=16)
                kept = [int(x) for x in r if int(x) != int(s)][:m] if int(s) in r else [int(x) for x in r[:m]]
                same = same and kept == [int(x) for x in rows[s - args.first] if x != 0xFFFFFFFF]
            dt = time.perf_counter() - t0
            emit(what="host_oracle_16_threads", sources_timed=hs, seconds=round(dt, 3), seconds_scaled_to_sources=round(dt * nsrc / hs, 1),
                 scaled_sources=nsrc, note="scaled linearly in sources from the timed ones", rows_equal_device=bool(same),
                 device_over_host=round(dt * nsrc / hs / best["seconds"], 1))
            assert same, "device lists and the oracle's differ"
        idx.close()
        del slab
        torch.cuda.empty_cache()
    if not args.trace and (args.only_searcher or not args.no_searcher):
        from frankensearch_amd.host import NativeTwoTierSearcher
        from frankensearch_amd.synthetic import random_bert_weights
        rng = np.random.default_rng(7)
        n = args.rows
        fslab, qslab = fixture(n, 256, 1, True), fixture(n, 384, 1, True)
        fast = fa.VectorIndex.from_device_slab(fslab.data_ptr(), n, 256, keepalive=fslab)
        qual = fa.VectorIndex.from_device_slab(qslab.data_ptr(), n, 384, keepalive=qslab)
        m2v = fa.Model2VecEmbedder(rng.standard_normal((5000, 256)).astype(np.float32))
        bert = fa.NativeEmbedder(random_bert_weights(5, 3000, 384, 6, 1536))
        s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, fast_tier_int8_multiplier=3)
        t0 = time.perf_counter()
        graph = fast.build_knn_graph(m)
        emit(what="fast_tier_graph", rows=n, dim=256, m=m, seconds=round(time.perf_counter() - t0, 3), mb=round(graph.nbytes / 1e6, 1))
        nq, kk = 1024, 10
        fq = [rng.integers(0, 5000, int(rng.integers(4, 24))).tolist() for _ in range(nq)]
        qq = [[101] + rng.integers(1000, 3000, int(rng.integers(6, 30))).tolist() + [102] for _ in range(nq)]
        res = {}
        for name, g in (("without_graph", None), ("with_graph", graph), ("without_graph_again", None)):
            s.set_neighbor_smoothing(g, 0.3, m)
            ts = []
            for rep in range(4):
                t0 = time.perf_counter()
                out = s.search_many(fq, qq, kk, None)
                ts.append(time.perf_counter() - t0)
            res[name] = (round(1e3 * float(np.median(ts[1:])), 2), out[0])
        changed = sum(a != b for a, b in zip(res["with_graph"][1], res["without_graph"][1]))
        emit(what="search_many_1024_queries", rows=n, ms_without_graph=res["without_graph"][0], ms_with_graph=res["with_graph"][0],
             ms_without_graph_again=res["without_graph_again"][0], initial_lists_changed=changed,
             detached_equals_before=bool(res["without_graph"][1] == res["without_graph_again"][1]))
        for h in (s, fast, qual, m2v, bert):
            h.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Lab timing of the query-hubness table build (fsgpu_index_compute_query_hubness, hubness_kernels.hip) on one MI355X, against the
host restatement (fsgpu_query_hubness, 16 threads) and of the query-time cost of the correction in fshost_two_tier_search_many.
Corpus: the bench generator's 10M x 384 and 10M x 256 f16 slabs, built in HBM; samples of 256 / 1,024 / 4,096 of its queries, kq 10.
Every device call is warmed up once, then timed with a host clock around the blocking C call.  The host restatement is timed on a
100k-row slice already in host memory and SCALED linearly in the number of rows (the job is embarrassingly parallel in rows); its
table is compared with the device's bit for bit on that slice.  Prints one JSON line per measurement.

    python scripts/bench_hubness.py [--rows 10000000] [--reps 3] [--out profiles/hubness/bench_hubness.jsonl]

One process can run everything (the default), but on a shared card every step gets a process and a time limit of its own, chained so
that a step that fails or runs over ends the series (--out appends with --append):

    out=profiles/hubness/bench_hubness.jsonl; : > $out
    for cfg in "384 256" "384 1024" "384 4096" "256 256" "256 1024" "256 4096"; do set -- $cfg
      timeout -k 10 180 python scripts/bench_hubness.py --dim $1 --nq $2 --out $out --append || exit $?
    done
    timeout -k 10 240 python scripts/bench_hubness.py --only-searcher --out $out --append || exit $?
    for cfg in "384 256" "384 1024" "384 4096" "256 256" "256 1024" "256 4096"; do set -- $cfg
      timeout -k 10 150 rocprofv3 --kernel-trace --stats --output-format csv -d trace_dim$1_nq$2 -- \
          python scripts/bench_hubness.py --trace --dim $1 --nq $2 || exit $?
    done
    python scripts/hubness_trace_summary.py trace_dim*_nq*     # one configuration per profiler run, two table builds in each
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

CLUSTERS, NOISE, KQ = 64, 0.30, 10
VALU_F32_TFLOPS = 157.3   # vector f32 spec of the MI355X (packed fma); a separate multiply and add reaches half of it


def timed_ms(fn, reps):
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return round(1e3 * float(np.median(ts)), 3), round(1e3 * min(ts), 3)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--dim", type=int, default=0)
    ap.add_argument("--nq", type=int, default=0)
    ap.add_argument("--host-rows", type=int, default=100_000)
    ap.add_argument("--no-searcher", action="store_true")
    ap.add_argument("--only-searcher", action="store_true")
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    dev = torch.device("cuda:0")
    lines = []

    def emit(**kw):
        lines.append(json.dumps(kw))
        print(lines[-1], flush=True)

    def fixture(n, dim, seed_base, as_f16):
        out = torch.empty((n, dim), dtype=torch.float16 if as_f16 else torch.float32, device=dev)
        check(_lib.lib().fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, seed_base, 1 if as_f16 else 0, out.data_ptr(), None))
        return out

    dims = [] if args.only_searcher else [args.dim] if args.dim else [384, 256]
    samples = [args.nq] if args.nq else [256, 1024, 4096]
    tables = {}
    for dim in dims:
        slab = fixture(args.rows, dim, 1, True)
        idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), args.rows, dim, keepalive=slab)
        queries = fixture(max(samples), dim, 0xDEAD0000, False).cpu().numpy()
        for nq in samples:
            q = np.ascontiguousarray(queries[:nq])
            call = lambda: idx.compute_query_hubness(q, KQ)
            table = call()
            if args.trace:
                call()
                continue
            p50, mn = timed_ms(call, args.reps)
            flop = 2.0 * args.rows * nq * dim
            emit(what="device_call", rows=args.rows, dim=dim, queries=nq, kq=KQ, reps=args.reps, ms_p50=p50, ms_min=mn,
                 tflops_unfused=round(flop / (mn * 1e-3) / 1e12, 2), fraction_of_unfused_roof=round(flop / (mn * 1e-3) / 1e12 / (VALU_F32_TFLOPS / 2), 3),
                 slab_gb=round(args.rows * dim * 2 / 1e9, 2), r_d_median=float(np.median(table)), r_d_max=float(table.max()))
            tables[(dim, nq)] = table
            if dim == 384:
                # the host restatement on a slice already in host memory, 16 threads, timed around the C call alone
                n = min(args.host_rows, args.rows)
                rows = slab[:n].float().cpu().numpy()
                dptr = (C.c_void_p * n)(*[rows.ctypes.data + i * dim * 4 for i in range(n)])
                qptr = (C.c_void_p * nq)(*[q.ctypes.data + j * dim * 4 for j in range(nq)])
                dlen, qlen = np.full(n, dim, np.uint32), np.full(nq, dim, np.uint32)
                out = np.zeros(n, np.float32)
                t0 = time.perf_counter()
                check(_lib.lib().fsgpu_query_hubness(C.addressof(dptr), dlen.ctypes.data, n, C.addressof(qptr), qlen.ctypes.data, nq, KQ, 0,
                                                     out.ctypes.data))
                ms = 1e3 * (time.perf_counter() - t0)
                same = bool(np.array_equal(out.view(np.uint32), table[:n].view(np.uint32)))
                emit(what="host_restatement_16_threads", rows_timed=n, dim=dim, queries=nq, kq=KQ, ms=round(ms, 1),
                     ms_scaled_to_rows=round(ms * args.rows / n, 1), scaled_rows=args.rows, note="scaled linearly in rows from the timed slice",
                     device_over_host=round(ms * args.rows / n / mn, 1), bits_equal_device_on_slice=same)
                assert same, "device and host tables differ on the slice"
        idx.close()
        del slab
        torch.cuda.empty_cache()
    if not args.trace and not args.no_searcher and (args.only_searcher or not args.dim):
        # query-time cost: fshost_two_tier_search_many over 1,024 queries with and without an attached table, same run
        from frankensearch_amd.host import NativeTwoTierSearcher
        from frankensearch_amd.synthetic import random_bert_weights
        rng = np.random.default_rng(7)
        fslab, qslab = fixture(args.rows, 256, 1, True), fixture(args.rows, 384, 1, True)
        fast = fa.VectorIndex.from_device_slab(fslab.data_ptr(), args.rows, 256, keepalive=fslab)
        qual = fa.VectorIndex.from_device_slab(qslab.data_ptr(), args.rows, 384, keepalive=qslab)
        m2v = fa.Model2VecEmbedder(rng.standard_normal((5000, 256)).astype(np.float32))
        bert = fa.NativeEmbedder(random_bert_weights(5, 3000, 384, 6, 1536))
        s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, fast_tier_int8_multiplier=3)
        nq, k = 1024, 10
        fq = [rng.integers(0, 5000, int(rng.integers(4, 24))).tolist() for _ in range(nq)]
        qq = [[101] + rng.integers(1000, 3000, int(rng.integers(6, 30))).tolist() + [102] for _ in range(nq)]
        table = tables.get((256, 1024))
        if table is None:   # a step of its own: the table of the fast tier against 1,024 of its queries
            table = fast.compute_query_hubness(np.ascontiguousarray(fixture(1024, 256, 0xDEAD0000, False).cpu().numpy()), KQ)
        res = {}
        for name, tab in (("without_table", None), ("with_table", table), ("without_table_again", None)):
            s.set_hubness(tab, 0.2)
            for _ in range(2):
                s.search_many(fq, qq, k, None)
            res[name] = timed_ms(lambda: s.search_many(fq, qq, k, None), 7)
        emit(what="search_many_1024_queries", rows=args.rows, k=k, beta=0.2, ms_p50_without_table=res["without_table"][0],
             ms_p50_with_table=res["with_table"][0], ms_p50_without_table_again=res["without_table_again"][0],
             ms_min_without_table=res["without_table"][1], ms_min_with_table=res["with_table"][1],
             note="python packing of the queries and unpacking of 2 x 1,024 x 10 hits included in both")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

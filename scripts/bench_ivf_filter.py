"""Lab timing of the IVF index's int8 list filter (fsgpu_ivf_set_list_filter; ivf_filter_kernels.hip) on one MI355X.
Prints one JSON line per measurement.  The corpora are scripts/bench_ivf.py's:

  --corpus bench        the bench generator's clustered f16 slab and f32 queries, built in HBM
  --corpus structured   `--clusters` centres inside a random 8-dimensional subspace, lifted to `--dim` dimensions, made on the host

  copy     what enabling the filter cost: the ordered copy's bytes, its device time, the whole call
  filter   per nprobe: `--nq` host queries per call with the filter on, with it off and through the exact batched search, the three
           interleaved in each round; the lone query on and off; the filter's own stats of a warm call (slots, overflow, int8 dots,
           exact dots left, device time per stage) and the share of the HBM rate the score and selection launches reach for the
           bytes they read; the answers of the two modes compared bit for bit
Every time is the median of `--reps` calls after a warm-up of the same shape, one process (host clock around blocking calls).

    python scripts/bench_ivf_filter.py --rows 1000000 --out profiles/ivf_filter/bench_ivf_filter.jsonl
    python scripts/bench_ivf_filter.py --rows 10000000 --nlist 4096 --out profiles/ivf_filter/bench_ivf_filter.jsonl --append
    python scripts/bench_ivf_filter.py --corpus structured --rows 1000000 --dim 64 --out profiles/ivf_filter/bench_ivf_filter.jsonl --append
"""
from __future__ import annotations

import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from bench_ivf import CLUSTERS, NOISE, interleaved_median_ms, structured  # noqa: E402

HBM_GBS = 8000.0   # the MI355X's nominal HBM rate, GB/s: the yardstick of the two launches' byte rates


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
    ap.add_argument("--nprobes", default="1,4,8,16,64")
    ap.add_argument("--nq", type=int, default=1024)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--append", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import time

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
    idx.search_batched(queries, k)   # (builds the index's int8 copy, probes the shapes)
    ivf = idx.build_ivf(nlist, iters=args.iters, n_train=args.n_train)
    t0 = time.perf_counter()
    ivf.set_list_filter(True)
    t_enable = time.perf_counter() - t0
    f = ivf.filter_stats()
    emit(what="copy", rows=n, dim=dim, nlist=nlist, rotated=f.rotated, copy_mb=round(f.copy_bytes / 1e6, 1), build_ms=round(f.build_ms, 3),
         copy_gbs=round((f.copy_bytes + n * dim) / (f.build_ms * 1e-3) / 1e9, 1) if f.build_ms else None, enable_seconds=round(t_enable, 3))

    def mode(on):
        ivf.set_list_filter(on)

    for p in nprobes:
        def batched_on():
            mode(True)
            return ivf.search_batched(queries, k, p)

        def batched_off():
            mode(False)
            return ivf.search_batched(queries, k, p)

        def lone_on():
            mode(True)
            return ivf.search(queries[0], k, p)

        def lone_off():
            mode(False)
            return ivf.search(queries[0], k, p)
        on_ms, off_ms, exact_ms, one_on_ms, one_off_ms = interleaved_median_ms(
            [batched_on, batched_off, lambda: idx.search_batched(queries, k), lone_on, lone_off], args.reps)
        off = batched_off()
        st_off = ivf.stats
        on = batched_on()
        st, f = ivf.stats, ivf.filter_stats()
        equal = bool((on[2] == off[2]).all() and (on[3] == off[3]).all() and all(
            (on[0][i, :on[2][i]] == off[0][i, :on[2][i]]).all() and
            (on[1][i, :on[2][i]].view(np.uint32) == off[1][i, :on[2][i]].view(np.uint32)).all() for i in range(args.nq)))
        pitch = (dim + 63) // 64 * 64
        # bytes the two launches move: the ordered rows once per 16-member tile and 4 bytes written per int8 dot; the selection reads
        # its slot's scores six times (the count, four digits, the compaction)
        score_bytes = f.rows_filtered * 4 + f.rows_streamed * pitch
        select_bytes = f.rows_filtered * 4 * 6
        emit(what="filter", rows=n, dim=dim, nlist=nlist, k=k, nprobe=p, nq=args.nq, answers_equal=equal,
             on_ms=round(on_ms, 3), off_ms=round(off_ms, 3), exact_batched_ms=round(exact_ms, 3), queries_per_s=round(args.nq / on_ms * 1e3, 1),
             over_filter_off=round(off_ms / on_ms, 3), over_exact_batched=round(exact_ms / on_ms, 3),
             lone_on_p50_ms=round(one_on_ms, 4), lone_off_p50_ms=round(one_off_ms, 4), lone_over_filter_off=round(one_off_ms / one_on_ms, 3),
             device_ms_on=round(st.device_ms, 3), device_ms_off=round(st_off.device_ms, 3), filter_ms=round(f.filter_ms, 3),
             select_ms=round(f.select_ms, 3), rescore_ms=round(f.rescore_ms, 3), launches=st.launches,
             queries_filtered=f.queries_filtered, slots_filtered=f.slots_filtered, slots_overflowed=f.slots_overflowed,
             scratch_ranges=f.scratch_ranges, rows_filtered_per_query=round(f.rows_filtered / args.nq, 1), rows_streamed=f.rows_streamed,
             rows_rescored_per_query=round(f.rows_rescored / args.nq, 1), share_rescored=round(f.rows_rescored / max(f.rows_filtered, 1), 4),
             score_gbs=round(score_bytes / (f.filter_ms * 1e-3) / 1e9, 1) if f.filter_ms else None,
             score_share_of_hbm=round(score_bytes / (f.filter_ms * 1e-3) / 1e9 / HBM_GBS, 4) if f.filter_ms else None,
             select_gbs=round(select_bytes / (f.select_ms * 1e-3) / 1e9, 1) if f.select_ms else None,
             select_share_of_hbm=round(select_bytes / (f.select_ms * 1e-3) / 1e9 / HBM_GBS, 4) if f.select_ms else None)
    ivf.close()
    idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

"""Lab timing of fsgpu_index_update_knn_graph (knn_update_kernels.hip, vector_index_knn_update.cpp) against a rebuild with
fsgpu_index_build_knn_graph on one MI355X.  Corpus: the bench generator's f16 slab, built in HBM and adopted, with synthetic doc ids
(fsgpu_lab_index_attach_synthetic_doc_ids); WAL rows come from the same generator under another seed.  One JSON line per measurement.

  headline   N rows, `--wal` WAL entries of which `--replace` supersede an existing document, compact(), then the update of the old
             table against the rebuild of the new index: both wall times (median of --reps calls, host arrays to host arrays), their
             ratio, the device's own time, join_ms and the class counts.  The two tables are compared, rows and similarity bits.
  sweep      no deletes; WAL entries = 0.1 %, 0.3 %, 1 %, 3 % of N, one compaction each, the old table being the rebuild of the step
             before: where the update stops beating the rebuild.  max_added_fraction = 1 forces the incremental path throughout.

The first search after a compaction rebuilds the int8 copy of the slab; a 1,024-source build pays for it before either side is timed.

    python scripts/bench_knn_update.py --rows 1000000 --m 16 --out profiles/knn_update/bench_knn_update.jsonl
    python scripts/bench_knn_update.py --rows 1000000 --m 16 --sweep --out profiles/knn_update/bench_knn_update.jsonl --append
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--wal", type=int, default=1000)
    ap.add_argument("--replace", type=int, default=500)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sweep", action="store_true")
    ap.add_argument("--fractions", default="0.001,0.003,0.01,0.03")
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

    def timed(fn, reps):
        out, ts = None, []
        for _ in range(reps):
            t0 = time.perf_counter()
            out = fn()
            ts.append(time.perf_counter() - t0)
        return out, float(np.median(ts)), ts

    n, dim, m = args.rows, args.dim, args.m
    rng = np.random.default_rng(1)
    slab = fixture(n, dim, 1, True)
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
    check(L.fsgpu_lab_index_attach_synthetic_doc_ids(idx._h))
    idx.build_knn_graph(m, n_rows=1024)                                  # warm-up: the int8 copy, the shapes
    old, t_first, _ = timed(lambda: idx.build_knn_graph(m, want_sims=True), 1)
    emit(what="build_before", rows=n, dim=dim, m=m, seconds=round(t_first, 4))

    def one_round(what, n_new, n_replace, seed):
        """n_new + n_replace WAL entries, a compaction, the update against the rebuild -> the rebuilt table"""
        nonlocal old
        n0 = idx.record_count()
        w = n_new + n_replace
        vec = fixture(w, dim, seed, False).cpu().numpy()
        ids = [f"doc-{int(i):09d}" for i in rng.choice(n, size=n_replace, replace=False)] + [f"{what}-{seed}-{i:07d}" for i in range(n_new)]
        idx.append_batch(list(zip(ids, vec)))
        t0 = time.perf_counter()
        idx.compact()
        t_compact = time.perf_counter() - t0
        n2o = idx.rewrite_sources()[0]
        idx.build_knn_graph(m, n_rows=1024)                              # the int8 copy of the new slab, for both sides
        upd, t_upd, all_upd = timed(lambda: idx.update_knn_graph(old[0], old[1], n2o, max_added_fraction=1.0, want_stats=True), args.reps)
        new, t_new, all_new = timed(lambda: idx.build_knn_graph(m, want_sims=True), max(args.reps - 1, 1))
        equal = bool((upd[0] == new[0]).all() and (upd[1].view(np.uint32) == new[1].view(np.uint32)).all())
        st = upd[2]
        emit(what=what, rows_before=n0, dim=dim, m=m, wal_entries=w, replacing=n_replace,
             added_fraction=round(st["added"] / st["rows"], 5), compact_seconds=round(t_compact, 4), update_seconds=round(t_upd, 4),
             rebuild_seconds=round(t_new, 4), rebuild_over_update=round(t_new / t_upd, 2), update_all=[round(t, 4) for t in all_upd],
             rebuild_all=[round(t, 4) for t in all_new], tables_equal=equal, **{k: (round(v, 3) if isinstance(v, float) else v) for k, v in st.items()})
        assert equal, "the updated table and the rebuilt table differ"
        old = new

    if not args.sweep:
        one_round("headline", args.wal - args.replace, args.replace, 2)
    else:
        for i, f in enumerate(float(x) for x in args.fractions.split(",")):
            one_round("sweep", max(int(round(f * n)), 1), 0, 3 + i)
    idx.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a" if args.append else "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()

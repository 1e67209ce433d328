"""Lab timing of fsgpu_index_compact / _vacuum / _wal_append_batch (compact_kernels.hip, vector_index_compact.cpp) on one MI355X.
Corpus: the bench generator's 10M x 384 f16 slab, built in HBM and adopted, with synthetic doc ids (fsgpu_lab_index_attach_synthetic_doc_ids).
Cases (--case):
    trigger   1,000 WAL entries + 5 % tombstones: the reference's default compaction trigger      (compact)
    vacuum    20 % tombstones: the vacuum trigger                                                  (vacuum)
    wal1m     1,000,000 WAL entries, a tenth of them new versions of main rows                     (compact)
    appends   fsgpu_index_wal_append x 1,000 against ONE fsgpu_index_wal_append_batch of 1,000, every entry superseding a main row
    old       the route without compaction, on 1M rows: every vector to the host, fsgpu_fsvi_write, fsgpu_index_open_fsvi
For a rewrite it reports the whole call, the library's own split (plan = merge + runs + upload + WAL encode; kernel = the launches
until done; tables; rebuild of derived copies), and — the yardstick, in the same process — hipMemcpyDtoD of the same number of
destination bytes, five times, with the ratio kernel / median copy next to the copies' own spread.  --nt: the kernel's stores carry the
non-temporal hint.  One JSON line per measurement; --out FILE appends.

Kernel times proper come from a profiler run of their own (one case per run):
    rocprofv3 --kernel-trace --stats --output-format csv -d trace_trigger -- python scripts/bench_compaction.py --case trigger --reps 1
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

CLUSTERS, NOISE = 64, 0.30


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", required=True, choices=["trigger", "vacuum", "wal1m", "appends", "old"])
    ap.add_argument("--rows", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=384)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--nt", action="store_true")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    dev = torch.device("cuda:0")
    n, dim = args.rows, args.dim
    rng = np.random.default_rng(1)

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            with open(args.out, "a") as f:
                f.write(line + "\n")

    slab = torch.empty((n, dim), dtype=torch.float16, device=dev)
    check(L.fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, 1, 1, slab.data_ptr(), None))

    def fresh_index():
        idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, keepalive=slab)
        check(L.fsgpu_lab_index_attach_synthetic_doc_ids(idx._h))
        check(L.fsgpu_lab_index_set_compact_nt_stores(idx._h, int(args.nt)))
        return idx

    def unit(m):
        v = rng.standard_normal((m, dim)).astype(np.float32)
        return v / np.linalg.norm(v, axis=1, keepdims=True)

    def batch_args(ids, vec):
        enc = [s.encode() for s in ids]
        ptrs = (C.c_char_p * len(enc))(*enc)
        lens = np.asarray([len(b) for b in enc], dtype=np.uint32)
        return enc, ptrs, lens, np.ascontiguousarray(vec)

    def append_batch(idx, ids, vec):
        enc, ptrs, lens, vec = batch_args(ids, vec)
        t0 = time.perf_counter()
        check(L.fsgpu_index_wal_append_batch(idx._h, len(enc), C.cast(ptrs, C.c_void_p), lens.ctypes.data, vec.ctypes.data, dim))
        return 1e3 * (time.perf_counter() - t0)

    def rewrite_times(idx):
        ms, counts = (C.c_double * 5)(), (C.c_uint64 * 3)()
        check(L.fsgpu_lab_index_last_rewrite(idx._h, ms, counts))
        return dict(plan_ms=round(ms[0], 3), kernel_ms=round(ms[1], 3), tables_ms=round(ms[2], 3), rebuild_ms=round(ms[4], 3),
                    runs=counts[0], launches=counts[1], dst_bytes=counts[2])

    def copy_yardstick(nbytes):
        ms = (C.c_double * 6)()
        check(L.fsgpu_lab_device_copy_ms(0, nbytes, 6, ms))
        t = sorted(ms[1:])   # the first is the warm-up
        return dict(copy_ms_median=round(t[2], 3), copy_ms_min=round(t[0], 3), copy_ms_max=round(t[-1], 3))

    if args.case in ("trigger", "vacuum", "wal1m"):
        for rep in range(args.reps):
            idx = fresh_index()
            if args.case == "trigger":
                idx.set_live(rng.random(n) >= 0.05)
                append_ms = append_batch(idx, [f"new-{i:07d}" for i in range(1000)], unit(1000))
            elif args.case == "vacuum":
                idx.set_live(rng.random(n) >= 0.20)
                append_ms = 0.0
            else:
                m = 1_000_000
                ids = [f"doc-{int(i):09d}" if j % 10 == 0 else f"new-{j:07d}" for j, i in enumerate(rng.integers(0, n, m))]
                append_ms = append_batch(idx, ids, unit(m))
            wal, tomb = idx.wal_record_count(), idx.tombstone_count()
            t0 = time.perf_counter()
            st = idx.vacuum() if args.case == "vacuum" else idx.compact()
            call_ms = 1e3 * (time.perf_counter() - t0)
            rt = rewrite_times(idx)
            rows_after = idx.record_count()
            idx.close()
            y = copy_yardstick(rt["dst_bytes"])
            emit(case=args.case, rep=rep, rows=n, dim=dim, wal_entries=wal, tombstones=tomb, rows_after=rows_after, nt_stores=args.nt,
                 call_ms=round(call_ms, 3), host_ms=round(rt["plan_ms"] + rt["tables_ms"], 3), append_batch_ms=round(append_ms, 3), **rt, **y,
                 kernel_over_copy=round(rt["kernel_ms"] / y["copy_ms_median"], 3),
                 copy_spread=round(y["copy_ms_max"] / y["copy_ms_min"], 3),
                 kernel_gbps=round(2 * rt["dst_bytes"] / rt["kernel_ms"] / 1e6, 1), copy_gbps=round(2 * rt["dst_bytes"] / y["copy_ms_median"] / 1e6, 1))
    elif args.case == "appends":
        picks = rng.choice(n, 2000, replace=False)
        ids_a, ids_b = [f"doc-{int(i):09d}" for i in picks[:1000]], [f"doc-{int(i):09d}" for i in picks[1000:]]
        va, vb = unit(1000), unit(1000)
        idx = fresh_index()
        enc = [s.encode() for s in ids_a]
        t0 = time.perf_counter()
        for b, v in zip(enc, va):
            check(L.fsgpu_index_wal_append(idx._h, b, len(b), v.ctypes.data, dim))
        one_by_one = 1e3 * (time.perf_counter() - t0)
        batch = append_batch(idx, ids_b, vb)
        assert idx.wal_record_count() == 2000 and idx.tombstone_count() == 2000
        idx.close()
        emit(case="appends", rows=n, dim=dim, entries=1000, wal_append_x1000_ms=round(one_by_one, 3), wal_append_batch_1000_ms=round(batch, 3),
             bitmap_bytes=(n + 63) // 64 * 8)
    else:
        m = min(n, 1_000_000)
        path = os.path.join(os.environ.get("TMPDIR", "/tmp"), f"bench_compaction_{os.getpid()}.fsvi")
        ids = [f"doc-{i:09d}".encode() for i in range(m)]
        ptrs = (C.c_char_p * m)(*ids)
        lens = np.full(m, 13, dtype=np.uint32)
        t0 = time.perf_counter()
        host = slab[:m].float().cpu().numpy()                      # every vector to the host, widened
        t1 = time.perf_counter()
        check(L.fsgpu_fsvi_write(path.encode(), b"bench", b"", dim, m, C.cast(ptrs, C.c_void_p), lens.ctypes.data, host.ctypes.data, 1, 0))
        t2 = time.perf_counter()
        re = fa.VectorIndex.open(path)
        t3 = time.perf_counter()
        assert re.record_count() == m
        re.close()
        os.remove(path)
        total = 1e3 * (t3 - t0)
        emit(case="old", rows_measured=m, dim=dim, pull_ms=round(1e3 * (t1 - t0), 1), write_ms=round(1e3 * (t2 - t1), 1), open_ms=round(1e3 * (t3 - t2), 1),
             total_ms=round(total, 1), scaled_to_rows=n, total_ms_scaled=round(total * n / m, 1), note="scaled linearly in rows from rows_measured")


if __name__ == "__main__":
    main()

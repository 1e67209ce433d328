"""Lab timing of the device-resident index builder (index_build_kernels.hip, index_builder.cpp) on one MI355X.
Corpus: the bench generator's f32 rows, built in HBM, with doc ids "doc-000000000" ...; F16 slabs, adds of 65,536 rows
(--add-rows: other sizes, to tell the cost of many small launches from the cost of the kernel's own schedule).

Per size (--sizes rows x dim, default 1,000,000x384 10,000,000x384 10,000,000x256), after one warm-up build, --reps alternating repeats
in the same process:
    new       fsgpu_index_builder_add_device per --add-rows rows + fsgpu_index_builder_finish, without a file and (--file) with one
    kernels   the library's own split: ingest and permute between events on the stream, bytes / s, and — the yardstick —
              hipMemcpyDtoD of the same read + written bytes (n * dim * 3 for the ingest of an F16 slab, the slab for the permute)
    today     today's route from the same vectors resident in HBM: download, fsgpu_fsvi_write, fsgpu_index_open_fsvi
              (--today-rows caps what is measured; larger sizes are scaled linearly and say so)
One JSON line per measurement; --out FILE appends.  Kernel times proper come from a profiler run of their own:
    rocprofv3 --kernel-trace --stats --output-format csv -d trace_index_build -- python scripts/bench_index_build.py --sizes 10000000x384 --reps 1 --no-today
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
    ap.add_argument("--sizes", nargs="+", default=["1000000x384", "10000000x384", "10000000x256"])
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--add-rows", type=int, default=65_536, help="rows per add call")
    ap.add_argument("--file", action="store_true", help="also time the build with the FSVI file written")
    ap.add_argument("--no-today", action="store_true")
    ap.add_argument("--today-rows", type=int, default=1_000_000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "index_build", "bench_index_build.jsonl"))
    args = ap.parse_args()
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    dev = torch.device("cuda:0")
    tmp = os.environ.get("TMPDIR", "/tmp")

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    def copy_yardstick(nbytes):
        """hipMemcpyDtoD of nbytes / 2 source bytes (read + written = nbytes)."""
        ms = (C.c_double * 6)()
        check(L.fsgpu_lab_device_copy_ms(0, nbytes // 2, 6, ms))
        t = sorted(ms[1:])   # the first is the warm-up
        return t[2], t[0], t[-1]

    for size in args.sizes:
        n, dim = (int(x) for x in size.lower().split("x"))
        src = torch.empty((n, dim), dtype=torch.float32, device=dev)
        check(L.fsgpu_bench_fixture_device(0, 0, n, dim, CLUSTERS, NOISE, 1, 0, src.data_ptr(), None))
        ids = [b"doc-%09d" % i for i in range(n)]
        batches = []
        for lo in range(0, n, args.add_rows):
            part = ids[lo:lo + args.add_rows]
            batches.append((lo, len(part), (C.c_char_p * len(part))(*part), np.full(len(part), 13, dtype=np.uint32)))

        def build(path):
            b = fa.IndexBuilder(dim, "bench", "", quantization=1)
            t0 = time.perf_counter()
            for lo, m, ptrs, lens in batches:
                check(L.fsgpu_index_builder_add_device(b._h, m, C.cast(ptrs, C.c_void_p), lens.ctypes.data, src.data_ptr() + lo * dim * 4, dim,
                                                       None, None))
            t1 = time.perf_counter()
            idx = b.finish(path)
            t2 = time.perf_counter()
            st = b.last_stats
            assert idx.record_count() == n
            idx.close()
            b.close()
            return 1e3 * (t1 - t0), 1e3 * (t2 - t1), st

        build(None)   # warm-up: code objects, allocator, the first touch of every page
        ingest_bytes, slab_bytes = n * dim * 6, n * dim * 2
        for rep in range(args.reps):
            for with_file in ([False, True] if args.file else [False]):
                path = os.path.join(tmp, f"bench_index_build_{os.getpid()}.fsvi") if with_file else None
                adds_ms, finish_ms, st = build(path)
                if path:
                    os.remove(path)
                ci, ci_min, ci_max = copy_yardstick(ingest_bytes)
                cp, cp_min, cp_max = copy_yardstick(2 * slab_bytes)
                host_ms = st.sort_ms + st.tables_ms
                emit(case="new", rows=n, dim=dim, add_rows=args.add_rows, rep=rep, file=with_file, adds_ms=round(adds_ms, 2), finish_ms=round(finish_ms, 2),
                     total_ms=round(adds_ms + finish_ms, 2), ingest_host_clock_ms=round(st.ingest_ms, 2), ingest_device_ms=round(st.ingest_device_ms, 3),
                     permute_device_ms=round(st.permute_device_ms, 3), ingest_gbps=round(ingest_bytes / st.ingest_device_ms / 1e6, 1),
                     permute_gbps=round(2 * slab_bytes / st.permute_device_ms / 1e6, 1), ingest_copy_ms=round(ci, 3),
                     permute_copy_ms=round(cp, 3), ingest_over_copy=round(st.ingest_device_ms / ci, 3),
                     permute_over_copy=round(st.permute_device_ms / cp, 3), copy_spread=round(max(ci_max / ci_min, cp_max / cp_min), 3),
                     sort_ms=round(st.sort_ms, 2), tables_ms=round(st.tables_ms, 2), file_ms=round(st.file_ms, 2),
                     host_share=round(host_ms / (adds_ms + finish_ms), 3), ingest_launches=st.ingest_launches,
                     permute_launches=st.permute_launches, chunks=st.chunks, peak_device_bytes=st.peak_device_bytes)
            if not args.no_today:
                m = min(n, args.today_rows)
                path = os.path.join(tmp, f"bench_index_build_today_{os.getpid()}.fsvi")
                ptrs = (C.c_char_p * m)(*ids[:m])
                lens = np.full(m, 13, dtype=np.uint32)
                t0 = time.perf_counter()
                host = src[:m].cpu().numpy()
                t1 = time.perf_counter()
                check(L.fsgpu_fsvi_write(path.encode(), b"bench", b"", dim, m, C.cast(ptrs, C.c_void_p), lens.ctypes.data, host.ctypes.data, 0, 0))
                t2 = time.perf_counter()
                re = fa.VectorIndex.open(path)
                t3 = time.perf_counter()
                assert re.record_count() == m
                re.close()
                os.remove(path)
                total = 1e3 * (t3 - t0)
                emit(case="today", rows_measured=m, dim=dim, rep=rep, pull_ms=round(1e3 * (t1 - t0), 1), write_ms=round(1e3 * (t2 - t1), 1),
                     open_ms=round(1e3 * (t3 - t2), 1), total_ms=round(total, 1), scaled_to_rows=n, total_ms_scaled=round(total * n / m, 1),
                     note="measured" if m == n else "scaled linearly in rows from rows_measured")
        del src
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()

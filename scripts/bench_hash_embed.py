"""Lab timing of the hash embedder (hash_embed_kernels.hip, hash_embedder.cpp) on one MI355X.

Workloads (ASCII, deterministic): 1,024 queries of ~6 tokens and 65,536 documents of ~200 tokens, each under JL-384, FNV-384 and
FNV-256.  Per workload and configuration, after 3 warm-up calls, the median (and min / max) of --reps >= 20 calls of
    stages    fsgpu_lab_hash_embed_stage_ms: fsgpu_hash_embed with the device's own time, between events on the embedder's stream,
              of {texts and offsets to the device, the kernel, vectors back to the host} — the copies are the yardstick that says
              whether a call is bound by PCIe
    call      the host's clock around fsgpu_hash_embed
    cpu       scripts/hash_embed_cpu.cpp (the reference's 8-chain loop restated in C++, -O3 -march=native) on --threads threads,
              --cpu-reps runs; its vectors must equal the GPU's in every bit
One JSON line per measurement; --out FILE appends."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)


def workload(n, tokens, seed):
    rng = np.random.default_rng(seed)
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    vocab = np.array(["".join(rng.choice(letters, int(k))) for k in rng.integers(2, 11, 20000)])
    counts = rng.integers(max(1, tokens - tokens // 4), tokens + tokens // 4 + 1, n)
    picks = rng.integers(0, vocab.size, int(counts.sum()))
    out, at = [], 0
    for c in counts:
        out.append(" ".join(vocab[picks[at:at + c]]).encode())
        at += c
    offsets = np.zeros(n + 1, dtype=np.uint32)
    offsets[1:] = np.cumsum([len(b) for b in out])
    return np.frombuffer(b"".join(out), dtype=np.uint8), offsets, int(counts.sum())


def cpu_library():
    so = os.path.join(tempfile.gettempdir(), f"hash_embed_cpu_{os.getuid()}.so")
    subprocess.check_call(["g++", "-O3", "-march=native", "-ffp-contract=off", "-std=c++17", "-shared", "-fPIC", "-pthread", "-o", so,
                           os.path.join(HERE, "hash_embed_cpu.cpp")])
    lib = C.CDLL(so)
    lib.hash_embed_cpu.restype = None
    lib.hash_embed_cpu.argtypes = [C.c_void_p, C.c_void_p, C.c_uint32, C.c_uint32, C.c_int, C.c_uint64, C.c_void_p, C.c_uint32]
    return lib


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=5)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workloads", nargs="+", default=["queries", "documents"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hash_embed", "bench_hash_embed.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 runs"
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.errors import check
    L = _lib.lib()
    cpu = cpu_library()

    def emit(**kw):
        line = json.dumps(kw)
        print(line, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(line + "\n")

    shapes = {"queries": (1024, 6, 11), "documents": (65536, 200, 12)}
    for name in args.workloads:
        n, tokens, seed = shapes[name]
        text, offsets, total_tokens = workload(n, tokens, seed)
        for label, dim, algorithm, jl in (("jl-384", 384, "jl", 1), ("fnv-384", 384, "fnv_modular", 0), ("fnv-256", 256, "fnv_modular", 0)):
            e = fa.HashEmbedder(dim, algorithm, 42)
            out = np.empty((n, dim), dtype=np.float32)
            stage = (C.c_float * 3)()
            bad = C.c_uint32()
            for _ in range(3):   # warm-up: code object, workspaces, the first touch of `out`
                check(L.fsgpu_lab_hash_embed_stage_ms(e._h, text.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, stage))
            h2d, kern, d2h, call = [], [], [], []
            for _ in range(args.reps):
                check(L.fsgpu_lab_hash_embed_stage_ms(e._h, text.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, stage))
                h2d.append(stage[0]); kern.append(stage[1]); d2h.append(stage[2])
            for _ in range(args.reps):
                t0 = time.perf_counter()
                check(L.fsgpu_hash_embed(e._h, text.ctypes.data, offsets.ctypes.data, n, out.ctypes.data, None, C.byref(bad)))
                call.append(1e3 * (time.perf_counter() - t0))
            ref = np.empty_like(out)
            cpu_ms = []
            for _ in range(args.cpu_reps + 1):   # (the first run is the warm-up)
                t0 = time.perf_counter()
                cpu.hash_embed_cpu(text.ctypes.data, offsets.ctypes.data, n, dim, jl, 42, ref.ctypes.data, args.threads)
                cpu_ms.append(1e3 * (time.perf_counter() - t0))
            same = bool(np.array_equal(out.view(np.uint32), ref.view(np.uint32)))
            k, c, copies = stats(kern), stats(call), stats([a + b for a, b in zip(h2d, d2h)])
            cm = stats(cpu_ms[1:])
            emit(workload=name, config=label, texts=n, tokens=total_tokens, text_bytes=int(text.size), vector_bytes=int(out.nbytes),
                 reps=args.reps, kernel_ms=k, copies_ms=copies, h2d_ms=stats(h2d), d2h_ms=stats(d2h), call_ms=c,
                 cpu_threads=args.threads, cpu_reps=args.cpu_reps, cpu_ms=cm, gpu_bits_equal_cpu=same,
                 kernel_tokens_per_s=round(total_tokens / k["median"] * 1e3), call_texts_per_s=round(n / c["median"] * 1e3),
                 cpu_texts_per_s=round(n / cm["median"] * 1e3), call_over_copies=round(c["median"] / copies["median"], 2),
                 cpu_over_call=round(cm["median"] / c["median"], 2))
            assert same, "the CPU restatement and the GPU disagree"
            e.close()


if __name__ == "__main__":
    main()

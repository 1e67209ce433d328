"""Kernel times of `rocprofv3 --kernel-trace --stats -- python scripts/bench_reranker.py --trace` (the rocpd database it writes), per
call: the trace holds, per shape, 5 x (rerank call, embed call); a rerank call starts at bert_embed_typed_ln_kernel, an embed call at
the embedder's embedding kernel.  Prints per shape the median kernel time of both calls, the rerank call's kernels, and the rerank
call's share of the f16 matrix-core peak (2.5 PF dense) computed from its FLOPs (shapes of MiniLM-L6: H 384, I 1536, 6 layers).

    python scripts/reranker_trace_summary.py <rr_results.db>
"""
import sqlite3
import sys
from collections import defaultdict

import numpy as np

SHAPES = [(100, 64), (100, 256), (100, 512), (1000, 256), (1, 24)]
H, I, L, PEAK = 384, 1536, 6, 2.5e15


def rerank_flops(n, s):
    t = n * s
    full = 2 * t * H * 3 * H + n * 4 * s * s * H + 2 * t * H * H + 4 * t * H * I   # one full layer
    last = 2 * t * H * 3 * H + n * 4 * s * H + n * (2 * H * H + 4 * H * I)           # QKV of all tokens; the rest for [CLS] rows
    return (L - 1) * full + last + n * (2 * H * H + 2 * H)


def main(db):
    c = sqlite3.connect(db)
    rows = c.execute("select name, duration from kernels order by start").fetchall()
    # a rerank call (one or more chunks) runs from a typed embedding kernel up to the embed call's first kernel: the embedder's
    # embedding (batch paths), its query stage (<= 32 tokens) or its one-launch docs kernel
    embed_start = ("bert_embed_ln", "bert_q_qkv_attn", "bert_docs_w")
    calls, cur = [], None
    for name, dur in rows:
        short = name.split("(")[0]
        if "bert_embed_typed_ln_kernel" in short and (cur is None or cur[0] == "embed"):
            cur = ["rerank", defaultdict(float)]
            calls.append(cur)
        elif any(k in short for k in embed_start) and cur is not None and cur[0] == "rerank":
            cur = ["embed", defaultdict(float)]
            calls.append(cur)
        if cur is not None:
            cur[1][short] += dur / 1e3   # ns -> us
    per_shape = len(calls) // len(SHAPES)
    for si, (n, s) in enumerate(SHAPES):
        seg = calls[si * per_shape:(si + 1) * per_shape]
        rr = [sum(k.values()) for kind, k in seg if kind == "rerank"]
        em = [sum(k.values()) for kind, k in seg if kind == "embed"]
        rr_med, em_med = float(np.median(rr)), float(np.median(em))
        fl = rerank_flops(n, s)
        print(f"== {n} pairs x {s} tokens: rerank kernels {rr_med:.1f} us (median of {len(rr)}), embed kernels {em_med:.1f} us; "
              f"rerank {fl / 1e9:.1f} GFLOP -> {fl / (rr_med * 1e-6) / 1e12:.1f} TFLOP/s = {fl / (rr_med * 1e-6) / PEAK:.3f} of 2.5 PF")
        last = [k for kind, k in seg if kind == "rerank"][-1]
        for name, us in sorted(last.items(), key=lambda kv: -kv[1]):
            print(f"   {us:9.1f} us  {name}")


if __name__ == "__main__":
    main(sys.argv[1])

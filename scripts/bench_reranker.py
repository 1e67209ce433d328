"""Lab timing of the GPU cross-encoder (fsgpu_reranker_score) against the embedder (fsgpu_bert_embed) on the SAME token layouts, in
one process on one MI355X.  MiniLM-L6 shape (384 / 1536 / 6, vocab 30522) with synthetic weights; every shape is warmed up first;
each call is timed with a host clock around the blocking C call (both return after a device synchronise).  Prints one JSON line per
shape; `--trace` runs each shape a few times only (for a rocprofv3 --kernel-trace --stats run of its own).

    python scripts/bench_reranker.py [--reps 20] [--trace]
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


def synthetic(seed, vocab=30522, hidden=384, layers=6, inter=1536, max_pos=512):
    rng = np.random.default_rng(seed)

    def t(*shape, s=0.05):
        return (rng.standard_normal(shape) * s).astype(np.float32)
    w = {"bert.embeddings.word_embeddings.weight": t(vocab, hidden, s=0.5), "bert.embeddings.position_embeddings.weight": t(max_pos, hidden, s=0.1),
         "bert.embeddings.token_type_embeddings.weight": t(2, hidden, s=0.1), "bert.embeddings.LayerNorm.weight": 1 + t(hidden, s=0.1),
         "bert.embeddings.LayerNorm.bias": t(hidden)}
    for i in range(layers):
        p = f"bert.encoder.layer.{i}."
        for n in ("query", "key", "value"):
            w[p + f"attention.self.{n}.weight"], w[p + f"attention.self.{n}.bias"] = t(hidden, hidden, s=0.08), t(hidden)
        w[p + "attention.output.dense.weight"], w[p + "attention.output.dense.bias"] = t(hidden, hidden), t(hidden)
        w[p + "attention.output.LayerNorm.weight"], w[p + "attention.output.LayerNorm.bias"] = 1 + t(hidden, s=0.1), t(hidden)
        w[p + "intermediate.dense.weight"], w[p + "intermediate.dense.bias"] = t(inter, hidden), t(inter)
        w[p + "output.dense.weight"], w[p + "output.dense.bias"] = t(hidden, inter), t(hidden)
        w[p + "output.LayerNorm.weight"], w[p + "output.LayerNorm.bias"] = 1 + t(hidden, s=0.1), t(hidden)
    w["bert.pooler.dense.weight"], w["bert.pooler.dense.bias"] = t(hidden, hidden, s=hidden ** -0.5), t(hidden)
    w["classifier.weight"], w["classifier.bias"] = t(1, hidden, s=0.2), t(1)
    return w


def layout(n_pairs, tokens, seed):
    rng = np.random.default_rng(seed)
    ids = rng.integers(1000, 30000, n_pairs * tokens).astype(np.int32)
    types = np.zeros(n_pairs * tokens, np.int32)
    for p in range(n_pairs):
        types[p * tokens + min(16, tokens - 1):(p + 1) * tokens] = 1   # a 14-token query segment, the rest is the document
    offsets = (np.arange(n_pairs + 1) * tokens).astype(np.uint32)
    return ids, types, offsets


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--trace", action="store_true")
    args = ap.parse_args()
    import frankensearch_amd as fa
    w = synthetic(1)
    rr = fa.NativeReranker(w, device=0)
    emb = fa.NativeEmbedder(w, device=0)
    shapes = [(100, 64), (100, 256), (100, 512), (1000, 256), (1, 24)]
    reps = 3 if args.trace else args.reps
    for n, s in shapes:
        ids, types, offs = layout(n, s, n * 1000 + s)
        out = np.empty((n, 384), np.float32)
        for _ in range(2):   # warm-up of both paths
            rr.score_flat(ids, types, offs)
            emb.embed_flat(ids, offs, out)
        tr, te = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            rr.score_flat(ids, types, offs)
            tr.append(time.perf_counter() - t0)
            t0 = time.perf_counter()
            emb.embed_flat(ids, offs, out)
            te.append(time.perf_counter() - t0)
        tr_ms, te_ms = 1e3 * np.median(tr), 1e3 * np.median(te)
        print(json.dumps({"pairs": n, "tokens_per_pair": s, "tokens": n * s, "reps": reps, "rerank_ms_p50": round(tr_ms, 3),
                          "rerank_ms_min": round(1e3 * min(tr), 3), "embed_ms_p50": round(te_ms, 3), "embed_ms_min": round(1e3 * min(te), 3),
                          "rerank_over_embed": round(tr_ms / te_ms, 3)}), flush=True)


if __name__ == "__main__":
    main()

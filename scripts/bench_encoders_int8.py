"""The MiniLM-class encoder in both linear formats (f16 default, int8_dynamic — DESIGN §3.8): 1 query, 256 and 1,024 queries
(8..32 tokens) and 32 x 512-token documents, ms per call at the C ABI's flat argument shape.  One JSON line per format.
`--only f16|int8_dynamic --shape docs|q256` times one format on one shape (for a kernel trace of it alone)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

import frankensearch_amd as fa
from frankensearch_amd.synthetic import random_bert_weights


def flatten(batch):
    offs = np.zeros(len(batch) + 1, dtype=np.uint32)
    offs[1:] = np.cumsum([len(b) for b in batch])
    return np.concatenate([np.asarray(b, dtype=np.int32) for b in batch]), offs


def timed(m, batch, reps, warm):
    ids, offs = flatten(batch)
    out = np.empty((len(batch), m.dimension()), np.float32)
    for _ in range(warm):
        m.embed_flat(ids, offs, out)
    t0 = time.perf_counter()
    for _ in range(reps):
        m.embed_flat(ids, offs, out)
    return (time.perf_counter() - t0) / reps * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["f16", "int8_dynamic"])
    ap.add_argument("--shape", choices=["q1", "q256", "q1024", "docs"])
    ap.add_argument("--reps", type=int, default=50)
    a = ap.parse_args()
    rng = np.random.default_rng(0)
    w = random_bert_weights(1, 30522, 384, 6, 1536)
    queries = [[101] + rng.integers(1000, 30000, int(rng.integers(6, 31))).tolist() + [102] for _ in range(1024)]
    docs = [[101] + rng.integers(1000, 30000, 510).tolist() + [102] for _ in range(32)]
    shapes = {"q1": queries[:1], "q256": queries[:256], "q1024": queries, "docs": docs}
    for fmt in ([a.only] if a.only else ["f16", "int8_dynamic"]):
        m = fa.NativeEmbedder(w, linear=fmt)
        row = {"linear": fmt}
        for name, batch in shapes.items():
            if a.shape and name != a.shape:
                continue
            reps = a.reps * (4 if name == "q1" else 1)
            row[f"{name}_ms"] = round(timed(m, batch, reps, 10), 4)
        print(json.dumps(row), flush=True)
        m.close()


if __name__ == "__main__":
    main()

"""Lab timing of the device WordPiece tokenizer (wordpiece_kernels.hip, wordpiece.cpp) on one MI355X, against
`tokenizers.encode_batch` on the same box.

Workloads (ASCII words over a synthetic 30,522-entry vocabulary, deterministic): 1,024 queries of ~8 words and 65,536 documents of
~200 words.  Per workload, after 3 warm-up calls, the median (and min / max) of --reps >= 20 calls of
    stages    fsgpu_lab_wordpiece_encode_stage_ms: fsgpu_wordpiece_encode with the device's own time, between events on the
              tokenizer's stream, of {texts in, the three kernels (with the host's read of the total between them), ids out}
    call      the host's clock around fsgpu_wordpiece_encode
    copy      a plain copy of the text bytes to the device and of as many ids back (torch, pageable memory, between events)
    host      tokenizers' encode_batch on --threads threads (RAYON_NUM_THREADS), --cpu-reps runs; its ids must equal the device's
    fused     Model2VecEmbedder.embed_texts (raw text in) against encode_batch + the flattening of its ids + embed_flat
One JSON line per workload; --out FILE appends."""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def vocabulary(rng, size=30522):
    import numpy as np
    letters = list("abcdefghijklmnopqrstuvwxyz")
    vocab = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"] + letters + ["##" + c for c in letters]
    seen = set(vocab)
    words = []
    while len(vocab) < size:
        w = "".join(rng.choice(letters, int(rng.integers(2, 9))))
        piece = "##" + w if rng.random() < 0.4 else w
        if piece not in seen:
            seen.add(piece)
            vocab.append(piece)
            if not piece.startswith("##"):
                words.append(w)
    return vocab, np.asarray(words)


def workload(rng, words, n, count):
    """n texts of about `count` words: three in four are vocabulary words, the rest random letters (pieces, some [UNK])."""
    import numpy as np
    letters = np.array(list("abcdefghijklmnopqrstuvwxyz"))
    other = np.array(["".join(rng.choice(letters, int(k))) for k in rng.integers(3, 12, 5000)])
    pool = np.concatenate([words[:15000], other])
    counts = rng.integers(max(1, count - count // 4), count + count // 4 + 1, n)
    picks = rng.integers(0, pool.size, int(counts.sum()))
    texts, at = [], 0
    for c in counts:
        texts.append(" ".join(pool[picks[at:at + c]]))
        at += c
    return texts, int(counts.sum())


def stats(xs):
    xs = sorted(xs)
    return dict(median=round(xs[len(xs) // 2], 4), min=round(xs[0], 4), max=round(xs[-1], 4))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--cpu-reps", type=int, default=3)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--workloads", nargs="+", default=["queries", "documents"])
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "wordpiece", "bench_wordpiece.jsonl"))
    args = ap.parse_args()
    assert args.reps >= 20, "the median of at least 20 runs"
    os.environ["RAYON_NUM_THREADS"] = str(args.threads)   # (read by tokenizers when its pool starts)
    os.environ.setdefault("TOKENIZERS_PARALLELISM", "true")
    import numpy as np
    import torch
    from tokenizers import Tokenizer
    import frankensearch_amd as fa
    from frankensearch_amd import _lib
    from frankensearch_amd.embed import _text_arrays
    from frankensearch_amd.errors import check
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from wordpiece_ref import tokenizer_json
    L = _lib.lib()
    rng = np.random.default_rng(2024)
    vocab, words = vocabulary(rng)
    text_json = tokenizer_json(vocab)
    hf = Tokenizer.from_str(text_json)
    t0 = time.perf_counter()
    tok = fa.WordPieceTokenizer.from_tokenizer_json(text_json)
    create_s = time.perf_counter() - t0
    m2v = fa.Model2VecEmbedder(rng.standard_normal((len(vocab), 256)).astype(np.float32))

    shapes = {"queries": (1024, 8), "documents": (65536, 200)}
    for name in args.workloads:
        n, count = shapes[name]
        texts, total_words = workload(rng, words, n, count)
        flat, offsets = _text_arrays(texts)
        cap = int(offsets[-1]) + 2 * n
        ids = np.zeros(cap, dtype=np.uint32)
        out_offsets = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(n, dtype=np.uint8)
        total, bad = C.c_uint64(), C.c_uint32()
        stage = (C.c_float * 3)()

        def lab():
            check(L.fsgpu_lab_wordpiece_encode_stage_ms(tok._h, flat.ctypes.data, offsets.ctypes.data, n, 1, 0, ids.ctypes.data, cap,
                                                        out_offsets.ctypes.data, stage))

        def call():
            check(L.fsgpu_wordpiece_encode(tok._h, flat.ctypes.data, offsets.ctypes.data, n, 1, 0, ids.ctypes.data, cap,
                                           out_offsets.ctypes.data, status.ctypes.data, C.byref(total), C.byref(bad)))

        for _ in range(3):
            lab()
        h2d, kern, d2h, whole = [], [], [], []
        for _ in range(args.reps):
            lab()
            h2d.append(stage[0]); kern.append(stage[1]); d2h.append(stage[2])
        for _ in range(args.reps):
            t0 = time.perf_counter()
            call()
            whole.append(1e3 * (time.perf_counter() - t0))
        n_ids = int(total.value)
        assert not status.any()
        # the host tokenizer on the same texts
        host_ms, enc = [], None
        for _ in range(args.cpu_reps + 1):   # (the first run is the warm-up)
            t0 = time.perf_counter()
            enc = hf.encode_batch(texts)
            host_ms.append(1e3 * (time.perf_counter() - t0))
        same = n_ids == sum(len(e.ids) for e in enc) and all(
            np.array_equal(ids[out_offsets[i]:out_offsets[i + 1]], np.asarray(e.ids, dtype=np.uint32)) for i, e in enumerate(enc))
        # a plain copy of the text in and of as many ids out
        src = torch.from_numpy(flat.copy())
        back = torch.zeros(n_ids, dtype=torch.int32, device="cuda")
        copy_ms = []
        for i in range(3 + args.reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            dev = src.cuda()
            host = back.cpu()
            e1.record()
            torch.cuda.synchronize()
            if i >= 3:
                copy_ms.append(e0.elapsed_time(e1))
        del dev, host
        # raw text -> vectors, fused against host tokenisation + embed_flat
        out = np.empty((n, 256), dtype=np.float32)
        fused_ms, split_ms = [], []
        for i in range(3 + args.reps):
            t0 = time.perf_counter()
            m2v.embed_texts(tok, texts, out=out)   # (with the Python-side join of the texts, as the split path pays for its own marshalling)
            if i >= 3:
                fused_ms.append(1e3 * (time.perf_counter() - t0))
        ref = np.empty_like(out)
        for i in range(args.cpu_reps + 1):
            t0 = time.perf_counter()
            enc2 = hf.encode_batch(texts, add_special_tokens=False)
            lens = np.fromiter((len(e.ids) for e in enc2), dtype=np.int64, count=n)
            o2 = np.zeros(n + 1, dtype=np.uint32)
            o2[1:] = np.cumsum(lens)
            f2 = np.fromiter((x for e in enc2 for x in e.ids), dtype=np.uint32, count=int(o2[-1]))
            m2v.embed_flat(f2, o2, out=ref)
            if i >= 1:
                split_ms.append(1e3 * (time.perf_counter() - t0))
        bits = bool(np.array_equal(out.view(np.uint32), ref.view(np.uint32)))
        k, c, h = stats(kern), stats(whole), stats(host_ms[1:])
        line = dict(workload=name, texts=n, words=total_words, text_bytes=int(offsets[-1]), ids=n_ids, vocab=len(vocab), reps=args.reps,
                    create_s=round(create_s, 2), h2d_ms=stats(h2d), kernels_ms=k, d2h_ms=stats(d2h), call_ms=c, plain_copy_ms=stats(copy_ms),
                    host_threads=args.threads, host_reps=args.cpu_reps, host_encode_batch_ms=h, ids_equal_host=bool(same),
                    fused_embed_texts_ms=stats(fused_ms), host_tokenise_plus_embed_flat_ms=stats(split_ms), fused_bits_equal=bits,
                    kernels_texts_per_s=round(n / k["median"] * 1e3), call_texts_per_s=round(n / c["median"] * 1e3),
                    host_texts_per_s=round(n / h["median"] * 1e3), host_over_call=round(h["median"] / c["median"], 2))
        text = json.dumps(line)
        print(text, flush=True)
        if args.out:
            os.makedirs(os.path.dirname(args.out), exist_ok=True)
            with open(args.out, "a") as f:
                f.write(text + "\n")
        assert same, "the device's ids and tokenizers' disagree"
        assert bits, "the fused call and host tokenisation + embed_flat disagree"


if __name__ == "__main__":
    main()

"""numpy f32 restatement of the cross-encoder forward (TEST HELPER, not collected): BertForSequenceClassification with num_labels = 1
as the reference's NativeReranker runs it (crates/frankensearch-rerank/src/native.rs:956-1130): typed embeddings, every encoder
layer, the [CLS] row of the last one, pooled = tanh(W_p cls + b_p), logit = w_c . pooled + b_c, score = sigmoid(logit) (0 when the
logit is not finite).  Built from oracle.bert_oracle's helpers; the seeded pooler / classifier weights come from `head_weights`."""
from __future__ import annotations

import math
from typing import Dict, List, Sequence, Tuple

import numpy as np

from oracle.bert_oracle import ATTN_HEAD_DIM, attention, gelu, layer_norm, normalise_keys

F = np.float32
SCALE = F(0.17677669)


def head_weights(seed: int, hidden: int, scale: float = 1.0) -> Dict[str, np.ndarray]:
    """Seeded pooler + 1-row classifier in HF key layout."""
    rng = np.random.default_rng(seed)
    return {
        "bert.pooler.dense.weight": (rng.standard_normal((hidden, hidden)) * (1.0 / math.sqrt(hidden))).astype(F),
        "bert.pooler.dense.bias": (rng.standard_normal(hidden) * 0.05).astype(F),
        "classifier.weight": (rng.standard_normal((1, hidden)) * scale * 4.0 / math.sqrt(hidden)).astype(F),
        "classifier.bias": (rng.standard_normal(1) * 0.1).astype(F),
    }


def num_layers(weights: Dict[str, np.ndarray]) -> int:
    w = normalise_keys(weights)
    n = 0
    while f"bert.encoder.layer.{n}.attention.self.query.weight" in w:
        n += 1
    return n


def cls_rows(weights: Dict[str, np.ndarray], pairs: Sequence[Tuple[Sequence[int], Sequence[int]]]) -> np.ndarray:
    """[n, H] last-layer [CLS] rows (zeros for empty pairs)."""
    w = normalise_keys(weights)
    hidden = w["bert.embeddings.word_embeddings.weight"].shape[1]
    layers = num_layers(w)
    out = np.zeros((len(pairs), hidden), dtype=F)
    for d, (ids, types) in enumerate(pairs):
        n = len(ids)
        if n == 0:
            continue
        ids = np.asarray(ids, dtype=np.int64)
        types = np.asarray(types, dtype=np.int64)
        x = (w["bert.embeddings.word_embeddings.weight"][ids] + w["bert.embeddings.position_embeddings.weight"][np.arange(n)]).astype(F)
        x = layer_norm(x + w["bert.embeddings.token_type_embeddings.weight"][types], w["bert.embeddings.LayerNorm.weight"],
                       w["bert.embeddings.LayerNorm.bias"])
        for layer in range(layers):
            p = f"bert.encoder.layer.{layer}"
            wq = np.concatenate([w[f"{p}.attention.self.query.weight"], w[f"{p}.attention.self.key.weight"],
                                 w[f"{p}.attention.self.value.weight"]], axis=0)
            bq = np.concatenate([w[f"{p}.attention.self.query.bias"], w[f"{p}.attention.self.key.bias"],
                                 w[f"{p}.attention.self.value.bias"]], axis=0)
            qkv = (x @ wq.T + bq).astype(F)
            ctx = attention(qkv, hidden, SCALE)
            if layer == layers - 1:   # encoder_layer_cls: only the [CLS] row goes on
                x, ctx = x[:1], ctx[:1]
            attn = (ctx @ w[f"{p}.attention.output.dense.weight"].T + w[f"{p}.attention.output.dense.bias"]).astype(F)
            x = layer_norm(x + attn, w[f"{p}.attention.output.LayerNorm.weight"], w[f"{p}.attention.output.LayerNorm.bias"])
            inter = gelu((x @ w[f"{p}.intermediate.dense.weight"].T + w[f"{p}.intermediate.dense.bias"]).astype(F))
            ffn = (inter @ w[f"{p}.output.dense.weight"].T + w[f"{p}.output.dense.bias"]).astype(F)
            x = layer_norm(x + ffn, w[f"{p}.output.LayerNorm.weight"], w[f"{p}.output.LayerNorm.bias"])
        out[d] = x[0]
    return out


def logits(weights: Dict[str, np.ndarray], pairs) -> np.ndarray:
    """[n] f32 logits; an empty pair's logit is 0 (forward_batch, native.rs:959-961)."""
    w = normalise_keys(weights)
    cls = cls_rows(w, pairs)
    pooled = np.tanh((cls @ w["bert.pooler.dense.weight"].T + w["bert.pooler.dense.bias"]).astype(F)).astype(F)
    out = (pooled @ w["classifier.weight"].reshape(1, -1).T).reshape(-1).astype(F) + w["classifier.bias"].reshape(-1)[0]
    for d, (ids, _) in enumerate(pairs):
        if len(ids) == 0:
            out[d] = F(0.0)
    return out.astype(F)


def scores_of(lg: np.ndarray) -> np.ndarray:
    """sigmoid(logit) when finite, else 0 (rerank_sync, native.rs:1631-1710)."""
    lg = np.asarray(lg, dtype=F)
    with np.errstate(over="ignore"):
        s = (F(1.0) / (F(1.0) + np.exp(-lg.astype(np.float64)))).astype(F)
    return np.where(np.isfinite(lg), s, F(0.0)).astype(F)


def make_pair(rng: np.random.Generator, vocab: int, q_len: int, d_len: int) -> Tuple[List[int], List[int]]:
    """[CLS] q [SEP] d [SEP] with types 0 for [CLS] q [SEP] and 1 for d [SEP] (ids 101 / 102 when the vocabulary has them)."""
    cls_id, sep_id = (101, 102) if vocab > 102 else (1, 2)
    q = list(rng.integers(3, vocab, q_len))
    d = list(rng.integers(3, vocab, d_len))
    ids = [cls_id] + q + [sep_id] + d + [sep_id]   # (an empty document: [CLS] q [SEP] [SEP])
    types = [0] * (q_len + 2) + [1] * (len(ids) - q_len - 2)
    return [int(i) for i in ids], types


# ---- the rerank step after the model call (pipeline.rs:125-360), restated for the host tests --------------------------------
def _total_key(x: float) -> int:
    b = int(np.float32(x).view(np.int32))
    return b ^ ((b >> 31) & 0x7FFFFFFF)


def _total_key64(x: float) -> int:
    b = int(np.float64(x).view(np.int64))
    return b ^ ((b >> 63) & 0x7FFFFFFFFFFFFFFF)


def apply_ref(cands: List[dict], has_text: List[bool], scores: List[float], top_k: int, min_c: int, combine: int, k: float):
    """cands: dicts {doc_id (bytes), rerank_score (float, nan = None), ...}; returns (new list, applied)."""
    import functools
    n = len(cands)
    if n < min_c:
        return list(cands), False
    window = min(n, top_k)
    included = [i for i in range(window) if has_text[i]]
    if len(included) < min_c or len(scores) != len(included):
        return list(cands), False
    out = [dict(c) for c in cands]
    for i in range(window):
        out[i]["rerank_score"] = float("nan")
    for j, s in enumerate(scores):
        s = float(np.float32(s))
        if math.isfinite(s):
            out[included[j]]["rerank_score"] = s

    def skey(c):
        s = c["rerank_score"]
        return _total_key(s if math.isfinite(s) else -math.inf)

    def cmp(a, b):
        ka, kb = skey(a), skey(b)
        if ka != kb:
            return -1 if ka > kb else 1
        return (a["doc_id"] > b["doc_id"]) - (a["doc_id"] < b["doc_id"])

    win = out[:window]
    if combine == 0:
        win = sorted(win, key=functools.cmp_to_key(cmp))
    elif window >= 2:
        kf = 1.0 if math.isnan(k) else float(max(np.float32(k), np.float32(1.0)))
        order = sorted(range(window), key=functools.cmp_to_key(lambda a, b: cmp(win[a], win[b])))
        key = [0.0] * window
        for r, pos in enumerate(order):
            key[pos] = 1.0 / (kf + pos) + 1.0 / (kf + r)

        def cmp2(a, b):
            ka, kb = _total_key64(key[a]), _total_key64(key[b])
            if ka != kb:
                return -1 if ka > kb else 1
            da, db = win[a]["doc_id"], win[b]["doc_id"]
            return (da > db) - (da < db)
        order = sorted(order, key=functools.cmp_to_key(cmp2))
        win = [win[p] for p in order]
    return win + out[window:], True

"""Cross-encoder reranking — host-side mirror of the reference's NativeReranker (crates/frankensearch-rerank/src/native.rs:1240,
rerank_sync :1636-1710) and of the rerank step of its pipeline (rerank_step_with_combine, pipeline.rs:125-360) over libfsgpu.so.

Tokenisation and truncation stay with the caller: a pair is `[CLS] query [SEP] doc [SEP]` as token ids with their token-type ids.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .embed import _HF_LAYER_KEYS, _BertConfig, _BertLayerWeights, _BertWeights
from .errors import SearchError, check

PURE_REORDER = 0   # FSGPU_RERANK_PURE_REORDER: RerankCombine::PureReorder
RRF_COMBINE = 1    # FSGPU_RERANK_RRF_COMBINE: RerankCombine::RrfCombine { k }


class _RerankerWeights(C.Structure):
    _fields_ = [("bert", _BertWeights), ("type_vocab", C.c_uint32), ("pooler_w", C.c_void_p), ("pooler_b", C.c_void_p),
                ("classifier_w", C.c_void_p), ("classifier_b", C.c_void_p)]


class _Candidate(C.Structure):
    _fields_ = [("doc_id", C.c_char_p), ("doc_id_len", C.c_uint32), ("score", C.c_float), ("rerank_score", C.c_float),
                ("index", C.c_uint32)]


@dataclass
class RerankScore:
    """RerankScore (crates/frankensearch-core/src/types.rs): raw_logit is None when the logit is not finite (score 0 then)."""
    doc_id: str
    score: float
    original_rank: int
    raw_logit: Optional[float]


@dataclass
class RerankCandidate:
    """The fields of a ScoredResult the rerank step reads and writes: doc id, fused score, rerank score (None = not reranked), and
    the caller's row index."""
    doc_id: str
    score: float
    rerank_score: Optional[float] = None
    index: int = 0


def _flatten(pairs: Sequence[Tuple[Sequence[int], Sequence[int]]]):
    n = len(pairs)
    offsets = np.zeros(n + 1, dtype=np.uint32)
    for i, (ids, types) in enumerate(pairs):
        if len(ids) != len(types):
            raise ValueError(f"pair {i}: {len(ids)} ids but {len(types)} type ids")
        offsets[i + 1] = offsets[i] + len(ids)
    total = max(int(offsets[-1]), 1)
    flat = np.zeros(total, dtype=np.int32)
    flat_t = np.zeros(total, dtype=np.int32)
    for i, (ids, types) in enumerate(pairs):
        flat[offsets[i]:offsets[i + 1]] = np.asarray(ids, dtype=np.int64)
        flat_t[offsets[i]:offsets[i + 1]] = np.asarray(types, dtype=np.int64)
    return flat, flat_t, offsets


class NativeReranker:
    """MiniLM-class cross-encoder (BertForSequenceClassification, num_labels = 1) on the GPU.

    `weights` is a dict of f32 arrays in the HuggingFace key layout (bare `embeddings.*` / `encoder.*` keys get the `bert.` prefix,
    as parse_weights does); `bert.pooler.dense.{weight,bias}` and `classifier.{weight,bias}` are required."""

    def __init__(self, weights: dict, device: int = 0, ln_eps: float = 1e-12):
        w = {}
        for k, v in weights.items():
            if k.startswith("embeddings.") or k.startswith("encoder."):
                k = "bert." + k
            w[k] = np.ascontiguousarray(v, dtype=np.float32)
        word = w["bert.embeddings.word_embeddings.weight"]
        pos = w["bert.embeddings.position_embeddings.weight"]
        types = w["bert.embeddings.token_type_embeddings.weight"]
        layers = 0
        while f"bert.encoder.layer.{layers}.attention.self.query.weight" in w:
            layers += 1
        hidden = word.shape[1]
        inter = w["bert.encoder.layer.0.intermediate.dense.weight"].shape[0]
        cls_w = w["classifier.weight"]
        if cls_w.size != hidden or w["classifier.bias"].size != 1:
            raise ValueError(f"classifier must have one output row of {hidden} values (num_labels = 1)")
        if w["bert.pooler.dense.weight"].shape != (hidden, hidden) or w["bert.pooler.dense.bias"].shape != (hidden,):
            raise ValueError("pooler must be [hidden, hidden] + [hidden]")
        cfg = _BertConfig(word.shape[0], hidden, layers, hidden // 32, inter, min(pos.shape[0], 512), ln_eps)
        lw = (_BertLayerWeights * layers)()
        for i in range(layers):
            for f, key in _HF_LAYER_KEYS.items():
                setattr(lw[i], f, w[f"bert.encoder.layer.{i}.{key}"].ctypes.data)
        bw = _BertWeights(word.ctypes.data, pos.ctypes.data, types.ctypes.data, w["bert.embeddings.LayerNorm.weight"].ctypes.data,
                          w["bert.embeddings.LayerNorm.bias"].ctypes.data, lw)
        rw = _RerankerWeights(bw, types.shape[0], w["bert.pooler.dense.weight"].ctypes.data, w["bert.pooler.dense.bias"].ctypes.data,
                              cls_w.ctypes.data, w["classifier.bias"].ctypes.data)
        h = C.c_void_p()
        check(_lib.lib().fsgpu_reranker_create(device, C.byref(cfg), C.byref(rw), C.byref(h)))
        self._h = h

    @classmethod
    def from_safetensors(cls, path: str, device: int = 0, ln_eps: float = 1e-12) -> "NativeReranker":
        """NativeReranker::load: the model file goes to the library as it is (fsgpu_reranker_create_safetensors)."""
        with open(path, "rb") as f:
            return cls.from_safetensors_bytes(f.read(), device=device, ln_eps=ln_eps)

    @classmethod
    def from_safetensors_bytes(cls, blob: bytes, device: int = 0, ln_eps: float = 1e-12) -> "NativeReranker":
        buf = np.frombuffer(blob, dtype=np.uint8)
        if buf.ctypes.data % 8:
            buf = np.require(buf.copy(), requirements=["ALIGNED"])
        self = cls.__new__(cls)
        h = C.c_void_p()
        check(_lib.lib().fsgpu_reranker_create_safetensors(device, buf.ctypes.data, buf.size, ln_eps, C.byref(h)))
        self._h = h
        return self

    @property
    def max_length(self) -> int:
        return int(_lib.lib().fsgpu_reranker_max_length(self._h))

    def score_pairs(self, pairs: Sequence[Tuple[Sequence[int], Sequence[int]]]) -> Tuple[np.ndarray, np.ndarray]:
        """(logits, scores) [n] f32 of pre-tokenised pairs (ids, type_ids); score = sigmoid(logit), 0 for a non-finite logit."""
        flat, flat_t, offsets = _flatten(pairs)
        return self.score_flat(flat, flat_t, offsets)

    def score_flat(self, ids: np.ndarray, type_ids: np.ndarray, offsets: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
        """The C ABI as a host holds it: concatenated int32 ids and type ids, uint32 offsets [n + 1]."""
        for a, dt in ((ids, np.int32), (type_ids, np.int32), (offsets, np.uint32)):
            if a.dtype != dt or not a.flags.c_contiguous:
                raise TypeError("ids / type_ids must be contiguous int32 and offsets contiguous uint32")
        n = offsets.shape[0] - 1
        logits = np.zeros(max(n, 0), dtype=np.float32)
        scores = np.zeros(max(n, 0), dtype=np.float32)
        check(_lib.lib().fsgpu_reranker_score(self._h, ids.ctypes.data, type_ids.ctypes.data, offsets.ctypes.data, n,
                                              logits.ctypes.data, scores.ctypes.data))
        return logits, scores

    def score_texts(self, tokenizer, query: str, docs: Sequence[str], max_length: Optional[int] = None) -> Tuple[np.ndarray, np.ndarray]:
        """(logits, scores) [n] of `[CLS] query [SEP] doc [SEP]` from raw text (native.rs:1652-1666): tokenised and truncated
        (longest_first to `max_length`; None: the tokenizer file's truncation, 0: none) on the device by `tokenizer`, a
        WordPieceTokenizer, and scored over the ids where they lie.  A flagged query or document raises with `.bad_text` set to the
        pair's index; nothing is scored."""
        from .embed import _call_with_bad_text, _text_arrays
        q = query if isinstance(query, (bytes, bytearray)) else str(query).encode("utf-8", "surrogatepass")
        qa = np.frombuffer(bytes(q) or b"\0", dtype=np.uint8)
        flat, offsets = _text_arrays(docs)
        n = offsets.shape[0] - 1
        logits = np.zeros(n, dtype=np.float32)
        scores = np.zeros(n, dtype=np.float32)
        _call_with_bad_text(_lib.lib().fsgpu_reranker_score_texts, self._h, tokenizer._h, qa.ctypes.data, len(q), flat.ctypes.data,
                            offsets.ctypes.data, n, tokenizer.max_length if max_length is None else int(max_length),
                            logits.ctypes.data, scores.ctypes.data)
        return logits, scores

    def rerank_token_ids(self, pairs: Sequence[Tuple[Sequence[int], Sequence[int]]], doc_ids: Sequence[str]) -> List[RerankScore]:
        """rerank_sync (native.rs:1636-1710) over pre-tokenised pairs: one RerankScore per document, in input order."""
        if len(pairs) != len(doc_ids):
            raise ValueError("one doc id per pair")
        logits, scores = self.score_pairs(pairs)
        out = []
        for rank, (doc, logit, score) in enumerate(zip(doc_ids, logits, scores)):
            finite = math.isfinite(float(logit))
            out.append(RerankScore(doc, float(score) if finite else 0.0, rank, float(logit) if finite else None))
        return out

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_reranker_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def rerank_apply(candidates: Sequence[RerankCandidate], has_text: Sequence[bool], scores: Sequence[float], top_k_rerank: int,
                 min_candidates: int, combine: int = PURE_REORDER, k: float = 60.0) -> Tuple[List[RerankCandidate], bool]:
    """fsgpu_rerank_apply: the step after the model call.  Returns the candidates in their new order (new objects; the inputs are
    not modified) and whether the step was applied."""
    n = len(candidates)
    if len(has_text) != n:
        raise ValueError(f"one has_text flag per candidate: {len(has_text)} for {n}")
    keep = [c.doc_id.encode("utf-8") for c in candidates]
    arr = (_Candidate * max(n, 1))()
    for i, c in enumerate(candidates):
        arr[i] = _Candidate(keep[i], len(keep[i]), c.score, float("nan") if c.rerank_score is None else c.rerank_score, i)
    ht = np.asarray([1 if t else 0 for t in has_text] or [0], dtype=np.uint8)
    sc = np.asarray(list(scores) or [0.0], dtype=np.float32)
    applied = C.c_uint8(0)
    check(_lib.lib().fsgpu_rerank_apply(arr, n, ht.ctypes.data, sc.ctypes.data, len(scores), top_k_rerank, min_candidates,
                                        combine, k, C.byref(applied)))
    out = []
    for i in range(n):
        src = candidates[arr[i].index]
        rs = float(arr[i].rerank_score)
        out.append(RerankCandidate(src.doc_id, src.score, None if math.isnan(rs) else rs, src.index))
    return out, bool(applied.value)


def rerank_step(reranker: NativeReranker, candidates: Sequence[RerankCandidate],
                pair_for: Callable[[str], Optional[Tuple[Sequence[int], Sequence[int]]]], top_k_rerank: int = 100,
                min_candidates: int = 5, combine: int = PURE_REORDER,
                k: float = 60.0) -> Tuple[List[RerankCandidate], bool, Optional[SearchError]]:
    """rerank_step_with_combine (pipeline.rs:125-360): scores the window's candidates that have a pair (`pair_for(doc_id)`, the
    reference's text_fn), then reorders through fsgpu_rerank_apply.  Returns (candidates, applied, error): a scoring error leaves the
    candidates as they were and is returned, not raised (the graceful failure of pipeline.rs:177-191)."""
    cands = list(candidates)
    if len(cands) < min_candidates:
        return cands, False, None
    window = min(len(cands), top_k_rerank)
    pairs, has_text = [], []
    for c in cands[:window]:
        p = pair_for(c.doc_id)
        has_text.append(p is not None)
        if p is not None:
            pairs.append(p)
    if len(pairs) < min_candidates:
        return cands, False, None
    try:
        _, scores = reranker.score_pairs(pairs) if pairs else (None, np.zeros(0, np.float32))
    except SearchError as e:
        return cands, False, e
    out, applied = rerank_apply(cands, has_text + [False] * (len(cands) - window), [float(s) for s in scores], top_k_rerank,
                                min_candidates, combine, k)
    return out, applied, None

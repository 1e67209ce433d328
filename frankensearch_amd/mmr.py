"""Maximum Marginal Relevance — mirror of `frankensearch_fusion::mmr` (crates/frankensearch-fusion/src/mmr.rs) and of the MMR
stage of TwoTierSearcher (searcher.rs:2696-2745) over the C ABI.

  MmrConfig     mmr.rs:43-66 (enabled False, lambda 0.7, candidate_pool 30)
  mmr_rerank    mmr.rs:103-251 on caller-supplied vectors, on the host (fsgpu_mmr_rerank; no device needed)
  mmr_step      the searcher's stage: reorders the head of a result list, leaves the tail; composes after rerank_step
The index-level forms (VectorIndex.mmr_rerank / mmr_rerank_batched / mmr_rerank_docs, TwoTierIndex.mmr_rerank) read the pool's
vectors from the slab on the device (mmr_kernels.hip)."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import check


class _MmrConfig(C.Structure):
    _fields_ = [("enabled", C.c_uint32), ("candidate_pool", C.c_uint32), ("lambda_", C.c_double), ("reserved", C.c_uint32 * 4)]


@dataclass
class MmrConfig:
    enabled: bool = False
    lambda_: float = 0.7
    candidate_pool: int = 30

    def _c(self) -> _MmrConfig:
        return _MmrConfig(1 if self.enabled else 0, min(max(int(self.candidate_pool), 0), 0xFFFFFFFF), float(self.lambda_))


def mmr_rerank(scores: Sequence[float], embeddings: Sequence[Sequence[float]], k: int, config: MmrConfig = None,
               want_sims: bool = False):
    """mmr_rerank(scores, embeddings, k, config) on the host.  Returns the selected indexes (and, with want_sims, the pool x pool
    f64 matrix of sim(i, j) as the selection reads it).  Vectors may differ in length (the reference's cosine_sim form)."""
    cfg = config or MmrConfig()
    if len(scores) != len(embeddings):
        raise ValueError("scores and embeddings must have the same length")
    n = len(scores)
    s = np.ascontiguousarray(scores, dtype=np.float64).reshape(-1)
    vecs = [np.ascontiguousarray(e, dtype=np.float32).reshape(-1) for e in embeddings]
    ptrs = (C.c_void_p * max(n, 1))(*[v.ctypes.data if v.size else None for v in vecs])
    lens = np.asarray([v.size for v in vecs] or [0], dtype=np.uint32)
    pool = min(n, cfg._c().candidate_pool)
    order = np.zeros(max(n, 1), dtype=np.uint32)
    count = C.c_uint32(0)
    sims = np.zeros((pool, pool), dtype=np.float64) if want_sims else None
    check(_lib.lib().fsgpu_mmr_rerank(s.ctypes.data if n else None, C.addressof(ptrs), lens.ctypes.data, n, k, float(cfg.lambda_),
                                      cfg._c().candidate_pool, order.ctypes.data, C.byref(count),
                                      sims.ctypes.data if want_sims and pool else None))
    got = order[:count.value].copy()
    return (got, sims) if want_sims else got


def mmr_step(results: Sequence, index, config: MmrConfig, row_of=None) -> Tuple[List, bool]:
    """The MMR stage of TwoTierSearcher::search (searcher.rs:2696-2745) on a ranked result list: items with .doc_id and .score
    (RerankCandidate, as rerank_step returns them) or (doc_id, score, ...) tuples.  `index` is a VectorIndex or a TwoTierIndex.  The
    first min(len, max(candidate_pool, 1)) results are reordered by MMR over their document vectors, the tail keeps its place.  Returns
    (results, applied); the list comes back as it was when MMR is disabled, the pool is smaller than two or a document has no vector.
    row_of(item) -> fast-tier row or None: only read by a TwoTierIndex over raw slabs, which have no doc-id table to resolve ids."""
    items = list(results)
    if config is None or not config.enabled or len(items) < 2:
        return items, False
    docs = []
    for r in items:
        doc_id, score = (r.doc_id, r.score) if hasattr(r, "doc_id") else (r[0], r[1])
        row = row_of(r) if row_of is not None else None
        docs.append((doc_id, float(score), 0xFFFFFFFF if row is None else int(row)))
    if hasattr(index, "mmr_rerank_docs"):
        order, applied = index.mmr_rerank_docs(docs, config)
    else:
        order, applied = index.mmr_rerank(docs, config)
    return ([items[i] for i in order], True) if applied else (items, False)

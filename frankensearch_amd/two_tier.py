"""SyncTwoTierSearcher — mirror of the reference's two-phase query flow over the GPU tier
(crates/frankensearch-fusion/src/sync_searcher.rs:616-943; fsfs shape: crates/frankensearch-fsfs/src/runtime.rs:8185-8355).

  phase 0 / "Initial":  fast embed (potion Model2Vec) -> fast-tier scan (fetch = k * candidate_multiplier) ->
                        RRF with the lexical list
  phase 1 / "Refined":  quality embed (MiniLM) -> the quality pool (sync_searcher.rs:810-818) -> blend -> RRF with the lexical
                        list again.  The pool is `Retrieved` (an independent quality-tier scan + blend_two_tier) only when the
                        quality tier's space identity is ATTESTED (an admitted FSVI v2 artifact); every FSVI v1 artifact takes
                        `RescoredFastPool`: TwoTierIndex::quality_scores_for_hits gather-rescores the fast pool on the quality
                        tier (two_tier.rs:1566-1631) and blend_two_tier_aligned blends it (blend.rs:213-294).
Lexical (BM25) search is the caller's: it stays on the CPU in the reference and is passed in as a ranked list.
Defaults follow TwoTierConfig (crates/frankensearch-core/src/config.rs:169-176)."""
from __future__ import annotations

import time
from dataclasses import dataclass, field
from typing import Callable, List, Optional, Sequence, Tuple

import numpy as np

import ctypes as C

from . import _lib, fusion
from .errors import DimensionMismatch, InvalidConfig, check

POOL_RETRIEVED = 0   # SyncQualityPool::Retrieved: attested quality tier (FSVI v2 admission) — independent retrieval
POOL_RESCORED = 1    # SyncQualityPool::RescoredFastPool: legacy / unattested pair (every FSVI v1 artifact)


@dataclass
class TwoTierConfig:
    quality_weight: float = 0.7
    rrf_k: float = 60.0
    candidate_multiplier: int = 3
    # 0 = exact f16 scan of the fast tier; n = search_top_k_int8_two_pass(query, fetch, n) — the reference's default with
    # n = FAST_TIER_MULT = 3 (crates/frankensearch-index/src/two_tier.rs:1318-1337; sync_searcher::search_fast_hits)
    fast_tier_int8_multiplier: int = 0
    quality_pool: int = POOL_RETRIEVED


class TwoTierIndex:
    """The fast / quality pairing of crates/frankensearch-index/src/two_tier.rs: QualityAlignment (:404-409, computed at open by
    the merge walk :750-866) and quality_scores_for_hits (:1566-1631), over fsgpu_alignment_* / fsgpu_quality_scores_for_hits."""
    NONE, ALIGNED, MAPPING = 0, 1, 2

    def __init__(self, fast_index, quality_index):
        """Both unsharded (VectorIndex) or both row-sharded handles (NativeShardedIndex: fsgpu_sharded_alignment_create /
        fsgpu_sharded_quality_scores_for_hits — SURVEY 8e: the tiers shard identically, re-scored rows go to their shards)."""
        from .index import NativeShardedIndex
        self.fast, self.quality = fast_index, quality_index
        self.sharded = isinstance(fast_index, NativeShardedIndex)
        if quality_index is None:   # a fast-only build (TwoTierIndexBuilder.finish without quality records): nothing to align
            self._a = None
            return
        if self.sharded != isinstance(quality_index, NativeShardedIndex):
            raise TypeError("a fast / quality pair is either two indexes or two sharded handles")
        h = C.c_void_p()
        create = _lib.lib().fsgpu_sharded_alignment_create if self.sharded else _lib.lib().fsgpu_alignment_create
        check(create(fast_index._h, quality_index._h, C.byref(h)))
        self._a = h.value

    def close(self) -> None:
        if getattr(self, "_a", None):
            _lib.lib().fsgpu_alignment_destroy(self._a)
            self._a = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def has_quality_index(self) -> bool:
        """False for a fast-only pair (TwoTierIndex::has_quality_index, two_tier.rs): only alignment_kind (NONE) and close apply."""
        return self.quality is not None

    def _need_quality(self, what: str) -> None:
        if self._a is None:
            raise InvalidConfig(f"{what}: the pair has no quality tier (a fast-only build)")

    def alignment_kind(self) -> int:
        if self._a is None:
            return self.NONE
        return int(_lib.lib().fsgpu_alignment_kind(self._a))

    def quality_row(self, fast_row: int) -> Optional[int]:
        self._need_quality("quality_row")
        r = int(_lib.lib().fsgpu_alignment_quality_row(self._a, fast_row))
        return None if r < 0 else r

    def unmatched_quality_docs(self) -> int:
        self._need_quality("unmatched_quality_docs")
        return int(_lib.lib().fsgpu_alignment_unmatched_quality_docs(self._a))

    def quality_scores_for_hits(self, query: Sequence[float], hits: Sequence[Tuple[str, float, int]]) -> List[Optional[float]]:
        self._need_quality("quality_scores_for_hits")
        q = np.ascontiguousarray(query, dtype=np.float32)
        arr, keep = fusion._pack(hits)
        scores = np.zeros(max(len(hits), 1), dtype=np.float32)
        present = np.zeros(max(len(hits), 1), dtype=np.uint8)
        fn = _lib.lib().fsgpu_sharded_quality_scores_for_hits if self.sharded else _lib.lib().fsgpu_quality_scores_for_hits
        check(fn(self.fast._h, self.quality._h, self._a, q.ctypes.data, q.size, arr, len(hits), scores.ctypes.data,
                 present.ctypes.data))
        return [float(scores[i]) if present[i] else None for i in range(len(hits))]

    def mmr_rerank(self, hits: Sequence[Tuple], config) -> Tuple[List[int], bool]:
        """fsgpu_two_tier_mmr_rerank: the searcher's MMR stage over (doc_id, score[, fast row]) in rank order — quality-tier vectors
        first, the fast tier's for a document without one.  Returns (order over the whole list, applied)."""
        self._need_quality("mmr_rerank")
        if self.sharded:
            raise TypeError("MMR over row-sharded handles is not supported: a pool's rows sit on several GPUs")
        cfg = config._c()
        arr, keep = fusion._pack([(h[0], h[1], h[2] if len(h) > 2 else 0xFFFFFFFF) for h in hits])
        order = np.zeros(max(len(hits), 1), dtype=np.uint32)
        applied = C.c_uint8(0)
        check(_lib.lib().fsgpu_two_tier_mmr_rerank(self.fast._h, self.quality._h, self._a, arr, len(hits), C.addressof(cfg),
                                                   order.ctypes.data, C.byref(applied)))
        return [int(i) for i in order[:len(hits)]], bool(applied.value)

    def quality_scores_for_hits_batched(self, queries: np.ndarray, hit_lists: Sequence[Sequence[Tuple[str, float, int]]]) -> List[List[Optional[float]]]:
        """fsgpu_quality_scores_for_hits_batched: quality_scores_for_hits for a chunk of queries, ONE gather launch (unsharded pairs)."""
        self._need_quality("quality_scores_for_hits_batched")
        q = np.ascontiguousarray(queries, dtype=np.float32)
        nq = len(hit_lists)
        assert q.ndim == 2 and q.shape[0] == nq and not self.sharded
        flat = [h for hits in hit_lists for h in hits]
        offs = np.zeros(nq + 1, dtype=np.uint32)
        offs[1:] = np.cumsum([len(h) for h in hit_lists])
        arr, keep = fusion._pack(flat)
        scores = np.zeros(max(len(flat), 1), dtype=np.float32)
        present = np.zeros(max(len(flat), 1), dtype=np.uint8)
        check(_lib.lib().fsgpu_quality_scores_for_hits_batched(self.fast._h, self.quality._h, self._a, q.ctypes.data, nq, q.shape[1], arr,
                                                               offs.ctypes.data, scores.ctypes.data, present.ctypes.data))
        return [[float(scores[i]) if present[i] else None for i in range(int(offs[j]), int(offs[j + 1]))] for j in range(nq)]


@dataclass
class TwoTierMetrics:
    fast_embed_ms: float = 0.0
    fast_search_ms: float = 0.0
    phase1_total_ms: float = 0.0     # library name of the Initial stage (config.rs:465-480)
    quality_embed_ms: float = 0.0
    quality_search_ms: float = 0.0
    blend_ms: float = 0.0
    phase2_total_ms: float = 0.0     # library name of the Refined stage


@dataclass
class SearchOutcome:
    initial_results: List[fusion.FusedHit]
    final_results: List[fusion.FusedHit]
    fast_hits: List[Tuple[str, float, int]]
    quality_hits: List[Tuple[str, float, int]]
    blended: List[Tuple[str, float, int]]
    metrics: TwoTierMetrics = field(default_factory=TwoTierMetrics)


class SyncTwoTierSearcher:
    def __init__(self, fast_index, quality_index, fast_embedder, quality_embedder,
                 doc_id_of: Callable[[int], str], config: Optional[TwoTierConfig] = None):
        self.fast_index, self.quality_index = fast_index, quality_index
        self.fast_embedder, self.quality_embedder = fast_embedder, quality_embedder
        self.doc_id_of = doc_id_of
        self.config = config or TwoTierConfig()
        self.pair = TwoTierIndex(fast_index, quality_index) if self.config.quality_pool == POOL_RESCORED else None

    def _hits(self, index, vec: np.ndarray, fetch: int, int8_multiplier: int = 0) -> List[Tuple[str, float, int]]:
        if int8_multiplier:
            return [(self.doc_id_of(h.index), h.score, h.index)
                    for h in index.search_top_k_int8_two_pass(vec, fetch, int8_multiplier)]
        rows, scores, counts = index.search_batch(vec, fetch)
        n = int(counts[0])
        return [(self.doc_id_of(int(rows[0, i])), float(scores[0, i]), int(rows[0, i])) for i in range(n)]

    def search(self, fast_token_ids: Sequence[int], quality_token_ids: Sequence[int], k: int,
               lexical: Optional[Sequence[Tuple[str, float]]] = None, mmr=None) -> SearchOutcome:
        """mmr: an MmrConfig; when enabled, the final results pass through the MMR stage (searcher.rs:2696-2745) over the pair's
        document vectors.  Absent or disabled, the outcome is exactly what it is without the argument."""
        cfg = self.config
        fetch = max(k * max(cfg.candidate_multiplier, 1), k)   # candidate_count (rrf.rs:113-115)
        m = TwoTierMetrics()
        lex = list(lexical or [])
        t0 = time.perf_counter()
        fast_vec = self.fast_embedder.embed_token_ids(fast_token_ids)
        t1 = time.perf_counter()
        fast_hits = self._hits(self.fast_index, fast_vec, fetch, cfg.fast_tier_int8_multiplier)
        t2 = time.perf_counter()
        initial = fusion.rrf_fuse(lex, fast_hits, k, 0, k=cfg.rrf_k)
        t3 = time.perf_counter()
        m.fast_embed_ms, m.fast_search_ms, m.phase1_total_ms = (t1 - t0) * 1e3, (t2 - t1) * 1e3, (t3 - t0) * 1e3
        quality_vec = self.quality_embedder.embed_token_ids(quality_token_ids)
        t4 = time.perf_counter()
        if self.pair is not None:   # RescoredFastPool: the fast pool re-scored on the quality tier (a gather, not a scan)
            scores = self.pair.quality_scores_for_hits(quality_vec, fast_hits)
            quality_hits = [(d, q, i) for (d, _, i), q in zip(fast_hits, scores) if q is not None]
            t5 = time.perf_counter()
            blended = fusion.blend_two_tier_aligned(fast_hits, scores, cfg.quality_weight)
        else:
            quality_hits = self._hits(self.quality_index, quality_vec, fetch)
            t5 = time.perf_counter()
            blended = fusion.blend_two_tier(fast_hits, quality_hits, cfg.quality_weight)
            fast_index_of = {d: i for d, _, i in fast_hits}
            blended = [(d, s, fast_index_of.get(d, 0xFFFFFFFF)) for d, s, _ in blended]   # sync_searcher.rs:880-891
        t6 = time.perf_counter()
        final = fusion.rrf_fuse(lex, blended, k, 0, k=cfg.rrf_k)
        t7 = time.perf_counter()
        m.quality_embed_ms, m.quality_search_ms = (t4 - t3) * 1e3, (t5 - t4) * 1e3
        m.blend_ms, m.phase2_total_ms = (t6 - t5) * 1e3, (t7 - t3) * 1e3
        if mmr is not None and mmr.enabled and len(final) > 1:
            from .mmr import mmr_step
            pair = self.pair or TwoTierIndex(self.fast_index, self.quality_index)
            final, _ = mmr_step([(h.doc_id, h.rrf_score, h) for h in final], pair, mmr, row_of=lambda t: t[2].semantic_index)
            final = [h[2] for h in final]
        return SearchOutcome(initial, final, fast_hits, quality_hits, blended, m)


class TwoTierIndexBuilder:
    """TwoTierIndexBuilder (crates/frankensearch-index/src/two_tier.rs:2003-2331) over the device-resident index builder
    (index_builder.IndexBuilder, fsgpu_index_builder_*): add_fast_record / add_quality_record / add_record, per-tier duplicate
    rejection (:2125-2132), "at least one fast-tier record is required" (:2241-2247), default embedder ids `fast-tier` /
    `quality-tier`, and finish() -> TwoTierIndex, writing vector.fast.idx / vector.quality.idx when a directory is given.

    As in the reference, dimension and duplicate errors are raised by the add that causes them, and the vectors themselves are
    judged by the writer: records are handed to the device builder in batches (`batch` records, and at finish), so a non-finite or
    zero-norm vector is refused there (InvalidConfig with `.bad_row` relative to that batch).  A refused batch is dropped whole:
    its records are forgotten, their ids may be added again, and the builder goes on with what was staged before it.
    add_*_records take a whole block.  Without a quality record finish() returns a fast-only pair (has_quality_index() is False):
    alignment_kind() is NONE and the calls that need a quality tier raise InvalidConfig.
    The files carry publication nonce 0, as write_fsvi writes it: the successor-nonce and install protocol of publish_tier
    (:2277-2301) is not part of this builder."""
    FAST_FILENAME, QUALITY_FILENAME = "vector.fast.idx", "vector.quality.idx"

    def __init__(self, device: int = 0, quantization: int = 1, chunk_rows: int = 0, batch: int = 4096):
        self.device, self.quantization, self.chunk_rows, self.batch = device, quantization, chunk_rows, batch
        self._ids = {"fast": "fast-tier", "quality": "quality-tier"}
        self._dim = {"fast": None, "quality": None}
        self._seen = {"fast": set(), "quality": set()}
        self._pending = {"fast": ([], []), "quality": ([], [])}
        self._builder = {"fast": None, "quality": None}

    def set_fast_embedder_id(self, embedder_id: str) -> "TwoTierIndexBuilder":
        self._ids["fast"] = embedder_id
        return self

    def set_quality_embedder_id(self, embedder_id: str) -> "TwoTierIndexBuilder":
        self._ids["quality"] = embedder_id
        return self

    def _flush(self, tier: str) -> None:
        ids, vecs = self._pending[tier]
        if not ids:
            return
        if self._builder[tier] is None:
            from .index_builder import IndexBuilder
            self._builder[tier] = IndexBuilder(self._dim[tier], self._ids[tier], "", device=self.device, quantization=self.quantization,
                                               reject_duplicates=True, chunk_rows=self.chunk_rows)
        self._pending[tier] = ([], [])
        try:
            self._builder[tier].add(ids, np.concatenate(vecs, axis=0))
        except Exception:
            self._seen[tier].difference_update(ids)   # all-or-nothing below: none of the batch was staged
            raise

    def _add(self, tier: str, doc_ids: Sequence[str], vectors) -> None:
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        v = v.reshape(len(doc_ids), -1)
        expected = self._dim[tier] if self._dim[tier] is not None else v.shape[1]
        if v.shape[1] != expected:
            raise DimensionMismatch(f"expected {expected}, found {v.shape[1]}")
        fresh = set()
        for d in doc_ids:
            if d in self._seen[tier] or d in fresh:
                raise InvalidConfig(f"duplicate doc_id in {tier} tier; each document must have a unique id")
            fresh.add(d)
        self._dim[tier] = expected
        self._seen[tier] |= fresh
        ids, vecs = self._pending[tier]
        ids.extend(doc_ids)
        vecs.append(v.copy())
        if len(ids) >= self.batch:
            self._flush(tier)

    def add_fast_record(self, doc_id: str, embedding: Sequence[float]) -> None:
        self._add("fast", [doc_id], np.asarray(embedding, dtype=np.float32)[None, :])

    def add_quality_record(self, doc_id: str, embedding: Sequence[float]) -> None:
        self._add("quality", [doc_id], np.asarray(embedding, dtype=np.float32)[None, :])

    def add_record(self, doc_id: str, fast_embedding: Sequence[float], quality_embedding: Optional[Sequence[float]] = None) -> None:
        self.add_fast_record(doc_id, fast_embedding)
        if quality_embedding is not None:
            self.add_quality_record(doc_id, quality_embedding)

    def add_fast_records(self, doc_ids: Sequence[str], vectors) -> None:
        self._add("fast", list(doc_ids), vectors)

    def add_quality_records(self, doc_ids: Sequence[str], vectors) -> None:
        self._add("quality", list(doc_ids), vectors)

    def finish(self, dir: Optional[str] = None) -> TwoTierIndex:
        import os
        if self._dim["fast"] is None:
            raise InvalidConfig("at least one fast-tier record is required")
        built = {}
        for tier, name in (("fast", self.FAST_FILENAME), ("quality", self.QUALITY_FILENAME)):
            if self._dim[tier] is None:
                built[tier] = None
                continue
            self._flush(tier)
            built[tier] = self._builder[tier].finish(None if dir is None else os.path.join(str(dir), name))
            self._builder[tier].close()
        return TwoTierIndex(built["fast"], built["quality"])

"""Graph ANN search over the exact k-NN table, with certified recall — the reference's `ann` feature over the C ABI.

  AnnIndex.search_batched / search   HnswIndex::knn_search_with_stats (crates/frankensearch-index/src/hnsw.rs:842-1330)
  AnnIndex.certify_ef                HnswIndex::certify_ef_search (hnsw.rs:1354-1386)
  AnnStats                           AnnSearchStats (hnsw.rs:266-297), summed over a call
  conformal_recall_lower_bound ...   recall_certificate.rs:50-230
The graph is the table of VectorIndex.build_knn_graph, searched with a beam (include/fsgpu.h, "graph ANN search"): the answer is a
pure function of the slab, the live bitmap, the table, the query and the parameters.  VectorIndex.build_ann builds both."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import check

APPROXIMATE = 0
UNDERFILLED = 1
EMPTY_DESPITE_INDEXED_POINTS = 2


class _AnnConfig(C.Structure):
    _fields_ = [("n_entry", C.c_uint32), ("degree", C.c_uint32), ("expand", C.c_uint32), ("max_iters", C.c_uint32),
                ("reserved", C.c_uint32 * 4)]


class _AnnStats(C.Structure):
    _fields_ = [("index_size", C.c_uint64), ("dimension", C.c_uint32), ("ef_search", C.c_uint32), ("k_requested", C.c_uint32),
                ("launches", C.c_uint32), ("queries", C.c_uint64), ("approximate", C.c_uint64), ("underfilled", C.c_uint64),
                ("empty_despite_indexed_points", C.c_uint64), ("rows_scored", C.c_uint64), ("steps", C.c_uint64),
                ("device_ms", C.c_double)]


class _CertifiedEf(C.Structure):
    _fields_ = [("ef_search", C.c_uint32), ("meets_target", C.c_uint32), ("certified_recall", C.c_double)]


@dataclass
class AnnConfig:
    n_entry: int = 1024
    degree: int = 0
    expand: int = 4
    max_iters: int = 64

    def _c(self) -> _AnnConfig:
        u32 = lambda v: min(max(int(v), 0), 0xFFFFFFFF)
        return _AnnConfig(u32(self.n_entry), u32(self.degree), u32(self.expand), u32(self.max_iters))


@dataclass
class AnnStats:
    index_size: int = 0
    dimension: int = 0
    ef_search: int = 0
    k_requested: int = 0
    launches: int = 0
    queries: int = 0
    approximate: int = 0
    underfilled: int = 0
    empty_despite_indexed_points: int = 0
    rows_scored: int = 0
    steps: int = 0
    device_ms: float = 0.0


@dataclass
class CertifiedEf:
    ef_search: int
    certified_recall: float
    meets_target: bool


def _stats(s: _AnnStats) -> AnnStats:
    return AnnStats(**{name: getattr(s, name) for name, _ in _AnnStats._fields_})


def _certified(c: _CertifiedEf) -> CertifiedEf:
    return CertifiedEf(int(c.ef_search), float(c.certified_recall), bool(c.meets_target))


def _f64(values) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(values, dtype=np.float64).ravel())


def conformal_recall_lower_bound(recalls: Sequence[float], alpha: float) -> float:
    r = _f64(recalls)
    return _lib.lib().fsgpu_conformal_recall_lower_bound(r.ctypes.data if r.size else None, r.size, float(alpha))


def mean_recall_lower_bound(recalls: Sequence[float], delta: float) -> float:
    r = _f64(recalls)
    return _lib.lib().fsgpu_mean_recall_lower_bound(r.ctypes.data if r.size else None, r.size, float(delta))


def mean_recall_lower_bound_bernstein(recalls: Sequence[float], delta: float) -> float:
    r = _f64(recalls)
    return _lib.lib().fsgpu_mean_recall_lower_bound_bernstein(r.ctypes.data if r.size else None, r.size, float(delta))


def _min_ef(fn, calibration, target, level) -> Optional[CertifiedEf]:
    if not calibration:
        return None
    samples = [_f64(r) for _, r in calibration]
    efs = np.asarray([int(ef) for ef, _ in calibration], dtype=np.uint32)
    ptrs = (C.c_void_p * len(samples))(*[s.ctypes.data if s.size else None for s in samples])
    lens = np.asarray([s.size for s in samples], dtype=np.uint64)
    out = _CertifiedEf()
    check(fn(efs.ctypes.data, ptrs, lens.ctypes.data, len(samples), float(target), float(level), C.byref(out)))
    return _certified(out)


def certified_min_ef(calibration: Sequence[Tuple[int, Sequence[float]]], target: float, alpha: float) -> Optional[CertifiedEf]:
    """The smallest ef whose conformal bound meets the target; else the best certifiable one.  None for an empty calibration."""
    return _min_ef(_lib.lib().fsgpu_certified_min_ef, calibration, target, alpha)


def certified_min_ef_mean(calibration: Sequence[Tuple[int, Sequence[float]]], target: float, delta: float) -> Optional[CertifiedEf]:
    return _min_ef(_lib.lib().fsgpu_certified_min_ef_mean, calibration, target, delta)


class AnnIndex:
    """A k-NN table resident on an index's device (fsgpu_ann).  The index must stay open while the handle is used; after a compaction
    or a vacuum that moved rows every call raises InvalidConfig."""

    def __init__(self, index, graph_rows: np.ndarray, config: Optional[AnnConfig] = None):
        g = np.ascontiguousarray(graph_rows, dtype=np.uint32)
        if g.ndim != 2:
            raise ValueError("graph_rows must be [rows, width]")
        cfg = (config or AnnConfig())._c()
        self._index = index
        self._h = C.c_void_p()
        check(_lib.lib().fsgpu_ann_create(index._h, g.ctypes.data if g.size else None, g.shape[0], g.shape[1], C.addressof(cfg),
                                          C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_ann_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def record_count(self) -> int:
        return _lib.lib().fsgpu_ann_record_count(self._h)

    def device(self) -> int:
        return _lib.lib().fsgpu_ann_device(self._h)

    @property
    def stats(self) -> AnnStats:
        """The stats of the last search or certify call."""
        s = _AnnStats()
        check(_lib.lib().fsgpu_ann_last_stats(self._h, C.byref(s)))
        return _stats(s)

    def search_batched(self, queries: np.ndarray, k: int, ef: int):
        """-> (rows [nq, k] u32, scores [nq, k] f32, counts [nq] u32, flags [nq] u32); entries past a count are unspecified."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, qlen = q.shape
        rows = np.full((nq, max(int(k), 1)), 0xFFFFFFFF, dtype=np.uint32)
        scores = np.full((nq, max(int(k), 1)), np.nan, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        flags = np.zeros(nq, dtype=np.uint32)
        check(_lib.lib().fsgpu_ann_search_batched(self._h, q.ctypes.data, nq, qlen, int(k), int(ef), rows.ctypes.data, scores.ctypes.data,
                                                  counts.ctypes.data, flags.ctypes.data, None))
        return rows[:, :k], scores[:, :k], counts, flags

    def search_batched_device(self, queries_ptr: int, nq: int, k: int, ef: int, out_rows_ptr: int, out_scores_ptr: int,
                              out_counts_ptr: int, out_flags_ptr: Optional[int] = None) -> None:
        """fsgpu_ann_search_batched_device_queries: queries [nq, dim] f32 and the outputs in the memory of the index's device."""
        check(_lib.lib().fsgpu_ann_search_batched_device_queries(self._h, queries_ptr, int(nq), self._index.dimension(), int(k), int(ef),
                                                                 out_rows_ptr, out_scores_ptr, out_counts_ptr, out_flags_ptr, None))

    def search(self, query: Sequence[float], k: int, ef: int):
        """One query -> (rows [count], scores [count], flag)."""
        q = np.ascontiguousarray(query, dtype=np.float32).ravel()
        rows = np.full(max(int(k), 1), 0xFFFFFFFF, dtype=np.uint32)
        scores = np.full(max(int(k), 1), np.nan, dtype=np.float32)
        count, flag = C.c_uint32(0), C.c_uint32(0)
        check(_lib.lib().fsgpu_ann_search(self._h, q.ctypes.data, q.size, int(k), int(ef), rows.ctypes.data, scores.ctypes.data,
                                          C.byref(count), C.byref(flag), None))
        return rows[:count.value].copy(), scores[:count.value].copy(), flag.value

    def certify_ef(self, queries: np.ndarray, candidate_efs: Sequence[int], k: int, target: float, alpha: float
                   ) -> Tuple[CertifiedEf, List[CertifiedEf]]:
        """certify_ef_search -> (chosen, sweep): the candidates in ascending ef up to the first whose conformal bound meets the target."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self._index.dimension():
            from .errors import DimensionMismatch
            raise DimensionMismatch(f"expected {self._index.dimension()}, found {q.shape[1]}")
        efs = np.asarray([int(e) for e in candidate_efs], dtype=np.uint32)
        sweep = (_CertifiedEf * max(efs.size, 1))()
        chosen = _CertifiedEf()
        n = C.c_uint32(0)
        check(_lib.lib().fsgpu_ann_certify_ef(self._h, q.ctypes.data if q.size else None, q.shape[0], efs.ctypes.data if efs.size else None,
                                              efs.size, int(k), float(target), float(alpha), C.byref(chosen), sweep, C.byref(n)))
        return _certified(chosen), [_certified(sweep[i]) for i in range(n.value)]

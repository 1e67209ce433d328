"""Inverted-file index over a VectorIndex: device k-means, probed-list search, certified nprobe — over the C ABI.

  IvfIndex(index, nlist, config, init_centroids)   fsgpu_ivf_create: spherical Lloyd k-means on the device, then the lists
  IvfIndex.search_batched / search                 the nprobe nearest lists scored exactly, with the underfill fallback
  IvfIndex.certify_nprobe                          fsgpu_ann_certify_ef with nprobe candidates
  IvfIndex.set_list_filter / filter_stats          the opt-in int8 matrix-core list filter: the same answers from fewer exact dots
  IvfIndex.centroids / lists                       the index itself: with iters 0 and 1 the assignment and the update alone
The index and every answer are pure functions of their inputs (include/fsgpu.h, "IVF index"); only recall is statistical, and it is
certified.  VectorIndex.build_ivf builds one."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Optional, Sequence, Tuple

import numpy as np

from . import _lib
from .ann import APPROXIMATE, EMPTY_DESPITE_INDEXED_POINTS, UNDERFILLED, CertifiedEf, _CertifiedEf, _certified  # noqa: F401
from .errors import check


class _IvfConfig(C.Structure):
    _fields_ = [("iters", C.c_uint32), ("reserved0", C.c_uint32), ("n_train", C.c_uint64), ("reserved", C.c_uint32 * 4)]


class _IvfBuildInfo(C.Structure):
    _fields_ = [("iterations", C.c_uint32), ("reserved0", C.c_uint32), ("rows_trained", C.c_uint64), ("rows_changed_last", C.c_uint64),
                ("empty_lists", C.c_uint64), ("largest_list", C.c_uint64), ("smallest_list", C.c_uint64), ("assign_ms", C.c_double),
                ("update_ms", C.c_double), ("lists_ms", C.c_double)]


class _IvfStats(C.Structure):
    _fields_ = [("index_size", C.c_uint64), ("dimension", C.c_uint32), ("nlist", C.c_uint32), ("nprobe", C.c_uint32),
                ("k_requested", C.c_uint32), ("launches", C.c_uint32), ("reserved0", C.c_uint32), ("queries", C.c_uint64),
                ("approximate", C.c_uint64), ("underfilled", C.c_uint64), ("empty_despite_indexed_points", C.c_uint64),
                ("lists_probed", C.c_uint64), ("rows_scored", C.c_uint64), ("device_ms", C.c_double)]


class _IvfFilterStats(C.Structure):
    _fields_ = [("mode", C.c_uint32), ("rotated", C.c_uint32), ("slot_cap", C.c_uint32), ("k_cap", C.c_uint32), ("scratch_cap", C.c_uint64),
                ("copy_bytes", C.c_uint64), ("build_ms", C.c_double), ("queries_filtered", C.c_uint64), ("queries_uncertified", C.c_uint64),
                ("calls_above_k_cap", C.c_uint64), ("slots_filtered", C.c_uint64), ("slots_overflowed", C.c_uint64),
                ("slots_above_scratch", C.c_uint64), ("scratch_ranges", C.c_uint64), ("rows_filtered", C.c_uint64),
                ("rows_rescored", C.c_uint64), ("filter_ms", C.c_double), ("select_ms", C.c_double), ("rescore_ms", C.c_double),
                ("rows_streamed", C.c_uint64), ("reserved", C.c_uint64 * 3)]


@dataclass
class IvfConfig:
    iters: int = 8
    n_train: int = 0

    def _c(self) -> _IvfConfig:
        return _IvfConfig(min(max(int(self.iters), 0), 0xFFFFFFFF), 0, min(max(int(self.n_train), 0), 0xFFFFFFFFFFFFFFFF))


@dataclass
class IvfBuildStats:
    iterations: int = 0
    rows_trained: int = 0
    rows_changed_last: int = 0
    empty_lists: int = 0
    largest_list: int = 0
    smallest_list: int = 0
    assign_ms: float = 0.0
    update_ms: float = 0.0
    lists_ms: float = 0.0


@dataclass
class IvfStats:
    index_size: int = 0
    dimension: int = 0
    nlist: int = 0
    nprobe: int = 0
    k_requested: int = 0
    launches: int = 0
    queries: int = 0
    approximate: int = 0
    underfilled: int = 0
    empty_despite_indexed_points: int = 0
    lists_probed: int = 0
    rows_scored: int = 0
    device_ms: float = 0.0


@dataclass
class IvfFilterStats:
    """fsgpu_ivf_filter_stats: of the last search or certify call."""
    mode: int = 0
    rotated: int = 0
    slot_cap: int = 0
    k_cap: int = 0
    scratch_cap: int = 0
    copy_bytes: int = 0
    build_ms: float = 0.0
    queries_filtered: int = 0
    queries_uncertified: int = 0
    calls_above_k_cap: int = 0
    slots_filtered: int = 0
    slots_overflowed: int = 0
    slots_above_scratch: int = 0
    scratch_ranges: int = 0
    rows_filtered: int = 0
    rows_rescored: int = 0
    filter_ms: float = 0.0
    select_ms: float = 0.0
    rescore_ms: float = 0.0
    rows_streamed: int = 0


LIST_FILTER_OFF, LIST_FILTER_INT8 = 0, 1


def _fields(cls, s):
    return cls(**{name: getattr(s, name) for name, _ in s._fields_ if not name.startswith("reserved")})


class IvfIndex:
    """Centroids and inverted lists resident on an index's device (fsgpu_ivf).  The index must stay open while the handle is used;
    after a compaction or a vacuum that moved rows, or a change of the hreduce order, every call raises InvalidConfig."""

    def __init__(self, index, nlist: int, config: Optional[IvfConfig] = None, init_centroids=None):
        cfg = (config or IvfConfig())._c()
        init = None
        if init_centroids is not None:
            init = np.ascontiguousarray(init_centroids, dtype=np.float32)
            if init.shape != (int(nlist), index.dimension()):
                raise ValueError("init_centroids must be [nlist, dimension]")
        self._index = index
        self._h = C.c_void_p()
        check(_lib.lib().fsgpu_ivf_create(index._h, min(max(int(nlist), 0), 0xFFFFFFFF), init.ctypes.data if init is not None else None,
                                          C.addressof(cfg), C.byref(self._h)))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_ivf_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def record_count(self) -> int:
        return _lib.lib().fsgpu_ivf_record_count(self._h)

    def device(self) -> int:
        return _lib.lib().fsgpu_ivf_device(self._h)

    def nlist(self) -> int:
        return _lib.lib().fsgpu_ivf_nlist(self._h)

    @property
    def stats(self) -> IvfStats:
        """The stats of the last search or certify call."""
        s = _IvfStats()
        check(_lib.lib().fsgpu_ivf_last_stats(self._h, C.byref(s)))
        return _fields(IvfStats, s)

    @property
    def build_stats(self) -> IvfBuildStats:
        s = _IvfBuildInfo()
        check(_lib.lib().fsgpu_ivf_build_stats(self._h, C.byref(s)))
        return _fields(IvfBuildStats, s)

    def set_list_filter(self, on) -> None:
        """fsgpu_ivf_set_list_filter: the int8 matrix-core list filter (True / LIST_FILTER_INT8) or the plain probed-list scan.  On
        first use the handle builds its cluster-ordered int8 copy (blocks).  Answers do not change, bit for bit."""
        mode = (LIST_FILTER_INT8 if on else LIST_FILTER_OFF) if isinstance(on, (bool, np.bool_)) else int(on)
        check(_lib.lib().fsgpu_ivf_set_list_filter(self._h, min(max(mode, 0), 0xFFFFFFFF)))

    @property
    def list_filter(self) -> bool:
        return _lib.lib().fsgpu_ivf_list_filter(self._h) != LIST_FILTER_OFF

    def filter_stats(self) -> IvfFilterStats:
        s = _IvfFilterStats()
        check(_lib.lib().fsgpu_ivf_last_filter_stats(self._h, C.byref(s)))
        return _fields(IvfFilterStats, s)

    def centroids(self) -> np.ndarray:
        """-> [nlist, dimension] f32, the final centroids."""
        out = np.zeros((self.nlist(), self._index.dimension()), dtype=np.float32)
        check(_lib.lib().fsgpu_ivf_centroids(self._h, out.ctypes.data))
        return out

    def lists(self) -> Tuple[np.ndarray, np.ndarray]:
        """-> (offsets [nlist + 1] u64, rows [offsets[-1]] u32): local row ids, ascending inside a list."""
        offsets = np.zeros(self.nlist() + 1, dtype=np.uint64)
        check(_lib.lib().fsgpu_ivf_lists(self._h, offsets.ctypes.data, None))
        rows = np.zeros(int(offsets[-1]), dtype=np.uint32)
        if rows.size:
            check(_lib.lib().fsgpu_ivf_lists(self._h, None, rows.ctypes.data))
        return offsets, rows

    def search_batched(self, queries: np.ndarray, k: int, nprobe: int):
        """-> (rows [nq, k] u32, scores [nq, k] f32, counts [nq] u32, flags [nq] u32); entries past a count are unspecified."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        nq, qlen = q.shape
        rows = np.full((nq, max(int(k), 1)), 0xFFFFFFFF, dtype=np.uint32)
        scores = np.full((nq, max(int(k), 1)), np.nan, dtype=np.float32)
        counts = np.zeros(nq, dtype=np.uint32)
        flags = np.zeros(nq, dtype=np.uint32)
        check(_lib.lib().fsgpu_ivf_search_batched(self._h, q.ctypes.data, nq, qlen, int(k), int(nprobe), rows.ctypes.data, scores.ctypes.data,
                                                  counts.ctypes.data, flags.ctypes.data, None))
        return rows[:, :k], scores[:, :k], counts, flags

    def search_batched_device(self, queries_ptr: int, nq: int, k: int, nprobe: int, out_rows_ptr: int, out_scores_ptr: int,
                              out_counts_ptr: int, out_flags_ptr: Optional[int] = None) -> None:
        """fsgpu_ivf_search_batched_device_queries: queries [nq, dim] f32 and the outputs in the memory of the index's device."""
        check(_lib.lib().fsgpu_ivf_search_batched_device_queries(self._h, queries_ptr, int(nq), self._index.dimension(), int(k), int(nprobe),
                                                                 out_rows_ptr, out_scores_ptr, out_counts_ptr, out_flags_ptr, None))

    def search(self, query: Sequence[float], k: int, nprobe: int):
        """One query -> (rows [count], scores [count], flag)."""
        q = np.ascontiguousarray(query, dtype=np.float32).ravel()
        rows = np.full(max(int(k), 1), 0xFFFFFFFF, dtype=np.uint32)
        scores = np.full(max(int(k), 1), np.nan, dtype=np.float32)
        count, flag = C.c_uint32(0), C.c_uint32(0)
        check(_lib.lib().fsgpu_ivf_search(self._h, q.ctypes.data, q.size, int(k), int(nprobe), rows.ctypes.data, scores.ctypes.data,
                                          C.byref(count), C.byref(flag), None))
        return rows[:count.value].copy(), scores[:count.value].copy(), flag.value

    def certify_nprobe(self, queries: np.ndarray, candidate_nprobes: Sequence[int], k: int, target: float, alpha: float
                       ) -> Tuple[CertifiedEf, List[CertifiedEf]]:
        """-> (chosen, sweep): the candidates in ascending nprobe up to the first whose conformal bound meets the target;
        CertifiedEf.ef_search carries nprobe."""
        q = np.ascontiguousarray(queries, dtype=np.float32)
        if q.ndim == 1:
            q = q[None, :]
        if q.shape[1] != self._index.dimension():
            from .errors import DimensionMismatch
            raise DimensionMismatch(f"expected {self._index.dimension()}, found {q.shape[1]}")
        probes = np.asarray([int(p) for p in candidate_nprobes], dtype=np.uint32)
        sweep = (_CertifiedEf * max(probes.size, 1))()
        chosen = _CertifiedEf()
        n = C.c_uint32(0)
        check(_lib.lib().fsgpu_ivf_certify_nprobe(self._h, q.ctypes.data if q.size else None, q.shape[0],
                                                  probes.ctypes.data if probes.size else None, probes.size, int(k), float(target), float(alpha),
                                                  C.byref(chosen), sweep, C.byref(n)))
        return _certified(chosen), [_certified(sweep[i]) for i in range(n.value)]

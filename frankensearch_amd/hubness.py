"""Query-hubness correction — mirror of `frankensearch_fusion::hubness` (crates/frankensearch-fusion/src/hubness.rs) over the C ABI.

  HubnessConfig          hubness.rs:36-58 (beta 0.2, kq 10)
  compute_query_hubness  hubness.rs:109-138 on caller-supplied vectors, on the host (fsgpu_query_hubness; no device needed)
  apply_hubness_penalty  hubness.rs:67-86, with correct_phase1_pool's sort by VectorHit::cmp_rank (searcher.rs:769-777)
The index-level forms (VectorIndex.compute_query_hubness, NativeShardedIndex.compute_query_hubness) build the table from the slab
on the device (hubness_kernels.hip); NativeTwoTierSearcher.set_hubness attaches it to the searcher."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import check
from .fusion import _pack


class _HubnessConfig(C.Structure):
    _fields_ = [("beta", C.c_float), ("kq", C.c_uint32), ("reserved", C.c_uint32 * 4)]


@dataclass
class HubnessConfig:
    beta: float = 0.2
    kq: int = 10

    def is_identity(self) -> bool:
        b = np.float32(self.beta)
        return not np.isfinite(b) or b <= 0

    def _c(self) -> _HubnessConfig:
        return _HubnessConfig(float(self.beta), min(max(int(self.kq), 0), 0xFFFFFFFF))


def compute_query_hubness(docs: Sequence[Sequence[float]], queries: Sequence[Sequence[float]], kq: int,
                          hreduce: int = _lib.HREDUCE_SSE2) -> np.ndarray:
    """compute_query_hubness(doc_vecs, query_sample, kq) on the host: one r_d per document.  Vectors may differ in length; every
    dot runs over the common prefix, as the reference's does."""
    dv = [np.ascontiguousarray(d, dtype=np.float32).reshape(-1) for d in docs]
    qv = [np.ascontiguousarray(q, dtype=np.float32).reshape(-1) for q in queries]
    dptr = (C.c_void_p * max(len(dv), 1))(*[v.ctypes.data if v.size else None for v in dv])
    qptr = (C.c_void_p * max(len(qv), 1))(*[v.ctypes.data if v.size else None for v in qv])
    dlen = np.asarray([v.size for v in dv] or [0], dtype=np.uint32)
    qlen = np.asarray([v.size for v in qv] or [0], dtype=np.uint32)
    out = np.zeros(len(dv), dtype=np.float32)
    check(_lib.lib().fsgpu_query_hubness(C.addressof(dptr), dlen.ctypes.data, len(dv), C.addressof(qptr), qlen.ctypes.data, len(qv),
                                         min(max(int(kq), 0), 0xFFFFFFFF), hreduce, out.ctypes.data if len(dv) else None))
    return out


def apply_hubness_penalty(hits: Sequence[Tuple[str, float, int]], table: Sequence[float], config: HubnessConfig = None,
                          resort: bool = True) -> List[Tuple[str, float, int]]:
    """(doc_id, score, index) hits -> the same hits with score - beta * table[index] (no penalty past the table's end), sorted by
    cmp_rank when resort; unchanged when the config is an identity."""
    cfg = (config or HubnessConfig())._c()
    arr, keep = _pack(hits)
    t = np.ascontiguousarray(table, dtype=np.float32).reshape(-1)
    applied = C.c_uint8(0)
    check(_lib.lib().fsgpu_apply_hubness_penalty(arr, len(hits), t.ctypes.data if t.size else None, t.size, C.addressof(cfg),
                                                 1 if resort else 0, C.byref(applied)))
    return [((arr[i].doc_id or b"").decode(), arr[i].score, arr[i].index) for i in range(len(hits))]

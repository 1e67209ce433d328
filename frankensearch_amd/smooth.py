"""k-NN graph diffusion — mirror of `frankensearch_fusion::smooth` (crates/frankensearch-fusion/src/smooth.rs) over the C ABI.

  SmoothConfig            smooth.rs:38-69 (alpha 0.3, m 10, mutual False)
  neighbor_smooth         smooth.rs:84-153, 176-248: the input order is kept
  neighbor_smooth_ranked  smooth.rs:265-276: ... then sorted by VectorHit::cmp_rank
Both are keyed by ROW (the hit's index) over a table of VectorIndex.build_knn_graph / NativeShardedIndex.build_knn_graph, not by
doc-id string as the reference's DocumentGraph is: a hit whose index lies past the table (a resident WAL entry) is isolated.
NativeTwoTierSearcher.set_neighbor_smoothing attaches a table to the searcher."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import List, Sequence, Tuple

import numpy as np

from . import _lib
from .errors import check
from .fusion import _pack


class _SmoothConfig(C.Structure):
    _fields_ = [("alpha", C.c_float), ("m", C.c_uint32), ("mutual", C.c_uint32), ("reserved", C.c_uint32 * 5)]


@dataclass
class SmoothConfig:
    alpha: float = 0.3
    m: int = 10
    mutual: bool = False

    def is_identity(self) -> bool:
        a = np.float32(self.alpha)
        return not np.isfinite(a) or a <= 0 or int(self.m) == 0

    def _c(self) -> _SmoothConfig:
        return _SmoothConfig(float(self.alpha), min(max(int(self.m), 0), 0xFFFFFFFF), 1 if self.mutual else 0)


def _smooth(hits, graph_rows, config, resort: bool) -> List[Tuple[str, float, int]]:
    cfg = (config or SmoothConfig())._c()
    arr, keep = _pack(hits)
    g = None if graph_rows is None else np.ascontiguousarray(graph_rows, dtype=np.uint32)
    if g is not None and g.ndim != 2:
        raise ValueError("graph_rows must be [rows, width]")
    applied = C.c_uint8(0)
    check(_lib.lib().fsgpu_neighbor_smooth(arr, len(hits), g.ctypes.data if g is not None and g.size else None,
                                           g.shape[0] if g is not None else 0, g.shape[1] if g is not None else 0, C.addressof(cfg),
                                           1 if resort else 0, C.byref(applied)))
    return [((arr[i].doc_id or b"").decode(), arr[i].score, arr[i].index) for i in range(len(hits))]


def neighbor_smooth(hits: Sequence[Tuple[str, float, int]], graph_rows, config: SmoothConfig = None) -> List[Tuple[str, float, int]]:
    """(doc_id, score, index) hits -> the same hits, in the same order, with (1 - alpha) * score + alpha * mean of the scores of the
    in-pool rows among the first m of graph_rows[index]; unchanged on an identity config, an empty graph or an empty pool."""
    return _smooth(hits, graph_rows, config, False)


def neighbor_smooth_ranked(hits: Sequence[Tuple[str, float, int]], graph_rows, config: SmoothConfig = None) -> List[Tuple[str, float, int]]:
    """neighbor_smooth followed by the sort by cmp_rank (score descending, NaN last, doc id ascending) that rank-based fusion needs."""
    return _smooth(hits, graph_rows, config, True)

"""A numpy restatement of the neighbour smoothing (include/fsgpu.h, fsgpu_neighbor_smooth; crates/frankensearch-fusion/src/smooth.rs)
and of the k-NN graph's self rule (fsgpu_index_build_knn_graph).  np.float32 scalars, one accumulator, row-keyed."""
from __future__ import annotations

import numpy as np

F32 = np.float32
PAD = 0xFFFFFFFF


def is_identity(alpha, m) -> bool:
    a = F32(alpha)
    return bool(not np.isfinite(a) or a <= 0 or int(m) == 0)


def total_key(x) -> int:
    """f32::total_cmp as an integer key."""
    b = int(np.array([x], dtype=F32).view(np.int32)[0])
    return b ^ 0x7FFFFFFF if b < 0 else b


def cmp_rank_sorted(hits):
    """VectorHit::cmp_rank (types.rs:101-133): score descending with NaN as -inf under total_cmp, doc id bytes ascending."""
    def key(h):
        s = F32(h[1])
        return (-total_key(F32(-np.inf) if np.isnan(s) else s), h[0].encode())
    return sorted(hits, key=key)


def neighbor_smooth(hits, graph, alpha=0.3, m=10, mutual=False, resort=False, counted=None):
    """hits: (doc_id, score, index) tuples; graph: uint32 [len, width] or None.  counted (a list, optional) receives per hit the
    rows of the neighbours that were averaged."""
    hits = [(d, F32(s), int(i)) for d, s, i in hits]
    if is_identity(alpha, m) or graph is None or len(hits) == 0:
        return hits
    g = np.asarray(graph, dtype=np.uint32)
    if g.ndim != 2 or g.shape[0] == 0 or g.shape[1] == 0:
        return hits
    glen, width = g.shape
    pool = {}
    for _, s, i in hits:
        pool[i] = s          # the last occurrence wins
    walk = min(int(m), width)
    a = F32(alpha)
    keep = F32(F32(1.0) - a)
    out = []
    with np.errstate(all="ignore"):
        for d, s, row in hits:
            total, count, used = F32(0.0), 0, []
            if row < glen:
                for e in range(walk):
                    nb = int(g[row, e])
                    if nb == PAD:
                        break
                    if nb not in pool:
                        continue
                    if mutual:
                        if nb >= glen or not any(int(x) == row for x in g[nb]):   # the direct definition: a linear scan
                            continue
                    total = F32(total + pool[nb])
                    count += 1
                    used.append(nb)
            mean = s if count == 0 else F32(total / F32(count))
            out.append((d, F32(F32(keep * s) + F32(a * mean)), row))
            if counted is not None:
                counted.append(used)
    return cmp_rank_sorted(out) if resort else out


def knn_from_topk(rows, self_row, m):
    """The self rule: `rows` is the row-level top-(m + 1) of the query 'row self_row' (possibly shorter); take self out if it is
    there, else drop the last entry; pad to m."""
    rows = [int(r) for r in rows][: m + 1]
    if self_row in rows:
        rows.remove(self_row)
    elif len(rows) == m + 1:
        rows.pop()
    return rows + [PAD] * (m - len(rows))

"""Cases of the gather scan's shape tests (test_gpu_multi_filter_shapes.py) and of the checks that need no GPU
(test_multi_filter_contract.py).  numpy only; the oracle comes in as an argument.

What filter_gather_scan_kernel (filter_gather_kernels.hip) does with a dimension: chunks = dim / 8, groups = chunks / 4 (a chunk per
lane of a quad), leftover = chunks % 4 (lane 0 alone, the `a == 0` loop); rows are staged gather_row_pitch(dim) bytes apart.  The
planner (filter_gather_supported) takes every multiple of 8 whose tile, queries and candidate buffers fit 160 KB of LDS."""
import numpy as np

TILE_ROWS, WAVES, MAX_K, LDS_BUDGET = 64, 4, 256, 160 * 1024   # kGatherTileRows, kWavesPerBlock, kGatherMaxK, kGatherLdsBudget


def row_pitch(dim):
    """gather_row_pitch: the row's bytes rounded up to 64 modulo 256."""
    return (dim * 2 + 255 - 64) // 256 * 256 + 64


def lds_bytes(dim, kcap):
    """filter_gather_lds_bytes: the tile, a query per wave, a candidate buffer of 2 kcap entries per wave, the tile's row ids."""
    return TILE_ROWS * row_pitch(dim) + WAVES * dim * 4 + WAVES * 2 * kcap * 8 + TILE_ROWS * 4


def gather_supported(dim, k):
    return dim >= 8 and dim % 8 == 0 and 1 <= k <= MAX_K and lds_bytes(dim, 64 if k <= 64 else 256) <= LDS_BUDGET


# The largest supported dimension per k tier, by the formulas above.  The tile is 64 x pitch and the pitch steps by 256 bytes every
# 128 dimensions (929 .. 1,056 -> 2,112 bytes; 801 .. 928 -> 1,856 bytes); queries cost 16 bytes a dimension; the buffers and row ids
# 4,352 bytes at k <= 64 and 16,640 bytes above.
#   k <= 64: dim 1,056 -> 135,168 + 16,896 +  4,352 = 156,416 <= 163,840;  dim 1,064 (pitch 2,368) -> 151,552 + 17,024 +  4,352 = 172,928
#   k  > 64: dim   928 -> 118,784 + 14,848 + 16,640 = 150,272 <= 163,840;  dim   936 (pitch 2,112) -> 135,168 + 14,976 + 16,640 = 166,784
MAX_DIM_K64, MAX_DIM_K256 = 1056, 928

# dim: (groups, leftover chunks) — no group at 8, 16, 24; a leftover everywhere but 768 and 928; pitches 64 .. 2,112 bytes
DIMS = {8: (0, 1), 16: (0, 2), 24: (0, 3), 40: (1, 1), 72: (2, 1), 200: (6, 1), 768: (24, 0), MAX_DIM_K256: (29, 0), MAX_DIM_K64: (33, 0)}
KS = (1, 10, 64, 65, 256)
SHAPES = [(d, k) for d in DIMS for k in KS if gather_supported(d, k)]               # every one is answered by the gather scan
REFUSED = [(MAX_DIM_K64 + 8, 10), (MAX_DIM_K64, 65), (MAX_DIM_K256 + 8, 256), (12, 10)]   # ... and none of these

N, ALLOWED = 8192, (120, 113, 127, 64)     # 2 tiles, the second one part full; below N / 50 = 163.84
GROUP_SIZES = (9, 5, 6, 1)                  # more than 4: a wave serves a second query of the group


def left_to_right(slab_u16, queries):
    x = np.ascontiguousarray(slab_u16).view(np.float16).astype(np.float32)
    out = np.zeros((len(queries), x.shape[0]), dtype=np.float32)
    for j in range(x.shape[1]):
        out = (out + (x[None, :, j] * queries[:, j, None]).astype(np.float32)).astype(np.float32)
    return out


def shape_case(oracle, dim, n=N, allowed=ALLOWED, group_sizes=GROUP_SIZES):
    """Clustered rows and queries; selective filters of `allowed` rows; tombstones set after the filters: a tenth of the corpus and
    five rows of every filter."""
    rng = np.random.default_rng(500 + dim)
    slab = oracle.clustered_corpus_f16(0, n, dim)
    masks = []
    for count in allowed:
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, count, replace=False)] = True
        masks.append(m)
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, n // 10, replace=False)] = False
    for m in masks:
        live[rng.choice(np.flatnonzero(m), 5, replace=False)] = False
    fq = rng.permutation(np.concatenate([np.full(c, f, dtype=np.int32) for f, c in enumerate(group_sizes)]))
    queries = np.stack([oracle.clustered_query(q, dim) for q in range(fq.size)]).astype(np.float32)
    return dict(slab=slab, masks=masks, live=live, fq=fq, queries=queries)


# ---- ties and non-finite scores inside a selective filter ----------------------------------------------------------------------------

TIE_ALLOWED, TIE_DUPS = 150, range(60, 71)      # list positions 60 .. 70: eleven equal rows across the tile boundary at 64
TIE_KS = (10, 64, 70, 256)                      # filter 0 ties around place 10, filter 1 around place 70


def tie_case(oracle, dim):
    """Two filters of 150 rows.  In each, rows hold +inf, -inf and NaN in component 3, and list positions 60 .. 70 hold copies of the
    one vector that stood near place 10 (filter 0) or 70 (filter 1) for the filter's first query, so its eleven copies straddle that
    place.  Queries 0-2 of a filter have a positive component 3, 3-5 a negative one, 6-8 a zero."""
    rng = np.random.default_rng(900 + dim)
    n = N
    slab = oracle.clustered_corpus_f16(0, n, dim).copy()
    nq = 9
    queries = np.stack([oracle.clustered_query(q, dim) for q in range(2 * nq)]).astype(np.float32)
    for f in range(2):
        q = queries[f * nq:(f + 1) * nq]
        q[0:3, 3] = np.abs(q[0:3, 3]) + np.float32(0.05)
        q[3:6, 3] = -np.abs(q[3:6, 3]) - np.float32(0.05)
        q[6:9, 3] = 0
    lists = rng.choice(n, 2 * TIE_ALLOWED, replace=False).reshape(2, TIE_ALLOWED)
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, n // 10, replace=False)] = False
    masks, dups = [], []
    for f in range(2):
        rows = np.sort(lists[f])
        live[rows[list(TIE_DUPS)]] = True
        special = rng.choice(np.delete(np.arange(TIE_ALLOWED), list(TIE_DUPS)), 12, replace=False)
        for j, pos in enumerate(special):
            slab[rows[pos], 3] = (0x7C00, 0xFC00, 0x7E00)[j % 3]     # +inf, -inf, NaN
        approx = slab[rows].view(np.float16).astype(np.float32) @ queries[f * nq]
        order = [p for p in np.argsort(-approx, kind="stable") if live[rows[p]] and p not in TIE_DUPS and p not in special]
        above = int(sum(1 for j, pos in enumerate(special) if j % 3 == 0 and live[rows[pos]]))   # the +inf rows lead query 0's answer
        source = rows[order[(10, 70)[f] - 6 - above]]   # its copies take the places from six before the 10th / 70th on
        slab[rows[list(TIE_DUPS)]] = slab[source]
        m = np.zeros(n, dtype=bool)
        m[rows] = True
        masks.append(m)
        dups.append(rows[list(TIE_DUPS)])
    fq = np.repeat(np.arange(2, dtype=np.int32), nq)
    return dict(slab=slab, masks=masks, live=live, fq=fq, queries=queries, dups=dups)

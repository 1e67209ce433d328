"""The k-NN graph optimisation of include/fsgpu.h (fsgpu_knn_graph_optimize) as a pure function in plain Python over
numpy tables: detour-count reordering, then reverse edges in (rank, source) order.  Nothing here is shared with the library.  The
keyword switches break ONE rule each; tests/test_knn_optimize_contract.py shows that every rule reaches the table."""
import numpy as np

PAD = 0xFFFFFFFF


def raw_lists(table):
    """Every row's columns before its first pad, as Python lists of global ids."""
    out = []
    for row in np.asarray(table, dtype=np.uint32).tolist():
        out.append(row[:row.index(PAD)] if PAD in row else row)
    return out


def clean_lists(table, row_base=0):
    """C(x): the raw list's ids that are rows of the table, not x itself and not kept before — as LOCAL rows."""
    n = len(table)
    out = []
    for x, raw in enumerate(raw_lists(table)):
        kept, have = [], set()
        for g in raw:
            r = g - row_base
            if 0 <= r < n and r != x and r not in have:
                have.add(r)
                kept.append(r)
        out.append(kept)
    return out


def detour_counts(table, row_base=0, p_le_i=False):
    """cnt[x][i]: the ranks j < i whose raw list holds C(x)[i]'s global id first at a column p < i."""
    raw = raw_lists(table)
    first = []   # global id -> first column, per row
    for lst in raw:
        at = {}
        for p, g in enumerate(lst):
            at.setdefault(g, p)
        first.append(at)
    clean = clean_lists(table, row_base)
    counts = []
    for c in clean:
        cnt = [0] * len(c)
        for i, y in enumerate(c):
            g = y + row_base
            for j in range(i):
                p = first[c[j]].get(g)
                if p is not None and (p <= i if p_le_i else p < i):
                    cnt[i] += 1
        counts.append(cnt)
    return clean, counts


def forward_lists(table, d, row_base=0, ties_desc=False, p_le_i=False):
    """F(x): C(x)'s ranks by (cnt ascending, i ascending), the first d — as local rows.  -> (F, max detour count)."""
    clean, counts = detour_counts(table, row_base, p_le_i)
    out, top = [], 0
    for c, cnt in zip(clean, counts):
        order = sorted(range(len(c)), key=lambda i: (cnt[i], -i if ties_desc else i))
        out.append([c[i] for i in order[:d]])
        if cnt:
            top = max(top, max(cnt))
    return out, top


def optimize(table, d, row_base=0, stats=None, ties_desc=False, p_le_i=False, reverse_desc=False, no_dedup=False, pad_mid=False):
    """-> [N, d] u32 global ids.  stats (a dict) receives the counts of fsgpu_knn_optimize_stats (all but device_ms)."""
    table = np.asarray(table, dtype=np.uint32)
    n, w = table.shape
    assert 1 <= d <= w <= 64
    fwd, top = forward_lists(table, d, row_base, ties_desc, p_le_i)
    rev = [[] for _ in range(n)]
    for r in range(d):   # rounds in ascending rank; inside a round sources ascending
        for x in (range(n - 1, -1, -1) if reverse_desc else range(n)):
            if r < len(fwd[x]) and len(rev[fwd[x][r]]) < d:
                rev[fwd[x][r]].append(x)
    h = (d + 1) // 2
    out = np.full((n, d), PAD, dtype=np.uint32)
    n_fwd = n_rev = 0
    for x in range(n):
        row = list(fwd[x][:h])
        origin = [0] * len(row)
        for cands, o in ((rev[x], 1), (fwd[x][h:], 0)):
            for y in cands:
                if len(row) >= d:
                    break
                if no_dedup or y not in row:
                    row.append(y)
                    origin.append(o)
        n_rev += sum(origin)
        n_fwd += len(origin) - sum(origin)
        if pad_mid and len(row) < d:   # the broken variant leaves the reverse half where it would be in a full row
            k = min(h, len(row))
            out[x, :k] = np.asarray(row[:k], dtype=np.int64) + row_base
            rest = row[k:]
            out[x, d - len(rest):d] = np.asarray(rest, dtype=np.int64) + row_base
        else:
            out[x, :len(row)] = np.asarray(row, dtype=np.int64) + row_base
    if stats is not None:
        stats.update(rows=n, forward_edges=n_fwd, reverse_edges=n_rev, max_detour_count=top,
                     zero_in_degree_before=zero_in_degree(table[:, :d], row_base), zero_in_degree_after=zero_in_degree(out, row_base))
    return out


def zero_in_degree(table, row_base=0):
    """Rows no walked edge points at: a list is walked to its first pad; an id outside the table or the row itself is no edge."""
    n = len(table)
    seen = np.zeros(n, dtype=bool)
    for x, raw in enumerate(raw_lists(table)):
        for g in raw:
            r = g - row_base
            if 0 <= r < n and r != x:
                seen[r] = True
    return int(n - seen.sum())


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

def structured_rows(rng, n, centres, basis):
    """Rows around the centres of a low-dimensional subspace, lifted by the basis, normalised, rounded through f16."""
    low = centres[rng.integers(0, centres.shape[0], n)] + 0.3 * rng.standard_normal((n, centres.shape[1]))
    x = (low @ basis).astype(np.float32)
    x = x / np.linalg.norm(x, axis=1, keepdims=True)
    return x.astype(np.float16).astype(np.float32)


def structured_corpus(seed=2, n=4096, nq=100, dim=64, sub=8, n_centres=32):
    """-> (rows [n, dim], queries [nq, dim]), f32 holding f16 values: 32 clusters inside a random 8-dimensional subspace."""
    rng = np.random.default_rng(seed)
    centres = rng.standard_normal((n_centres, sub))
    basis = rng.standard_normal((sub, dim))
    return structured_rows(rng, n, centres, basis), structured_rows(rng, nq, centres, basis)

"""The IVF index's contract (include/fsgpu.h, "IVF index") restated in plain Python: numpy, tests/ann_ref.py for the
certificate, and the CPU oracle — which comes in as an argument — for every score: oracle.gather_dot (row against centroid, row
against query) and oracle.search_top_k_f32 (query against the centroid matrix, i.e. dot_f32_bytes_f32 and the total order).  The
device returns all of it bit for bit.

`rules`: names of rules to BREAK, one at a time, for tests/test_ivf_contract.py — the empty set is the contract.
  ties_high      a tie between centroids goes to the higher id
  pairwise_sum   np.sum (pairwise) in the place of the sequential f64 sum
  no_normalise   the mean is stored as it is
  reseed_empty   a list without members takes the first training row's widening instead of keeping its centroid
  dead_at_build  the live bitmap of the build is used at search time (deletes made after the build are ignored)
  stride_k_tiles a probed list's best k are read k entries apart from a table that holds them 64 apart (k < 64, lists of one tile)
  stop_at_empty  an empty probed list ends the query's candidates: the lists probed after it are dropped
  first_launch   rows from LAUNCH_ROWS on (the assignment's second launch) are never assigned"""
import numpy as np

import ann_ref

F32 = np.float32
APPROXIMATE, UNDERFILLED, EMPTY = 0, 1, 2
LAUNCH_ROWS = 1 << 20   # kernels.hpp kIvfLaunchRows: rows per assignment launch
TILE_ROWS = 64          # kernels.hpp kGatherTileRows: a scan block's partial list is 64 entries wide for k <= 64


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def score_ord(scores):
    """f32::total_cmp as an unsigned key, with NaN as -inf (device_util.hpp score_ord)."""
    b = bits(scores).astype(np.uint32).copy()
    b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFF800000)
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint64)


def order_keys(scores, ids):
    """Greater is better: score descending, the lower id first."""
    return (score_ord(scores) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - np.asarray(ids, dtype=np.uint64))


def widen(slab_u16):
    return np.ascontiguousarray(slab_u16, dtype=np.uint16).view(np.float16).astype(F32)


def training_rows(n, n_train, live=None):
    rows = np.arange(n, dtype=np.int64) if (n_train == 0 or n_train >= n) else (np.arange(n_train, dtype=np.int64) * n) // n_train
    if live is not None:
        rows = rows[np.asarray(live, dtype=bool)[rows]]
    return rows


def strided_init(slab_u16, train, nlist):
    t = len(train)
    return widen(slab_u16)[train[(np.arange(nlist, dtype=np.int64) * t) // nlist]].copy()


def centroid_scores(oracle, slab_u16, centroids, hreduce=0):
    """[nlist, N]: row against centroid, fsgpu_gather_dot's bits."""
    n = slab_u16.shape[0]
    every = np.arange(n, dtype=np.uint32)
    return np.stack([oracle.gather_dot(slab_u16, c, every, hreduce) for c in np.ascontiguousarray(centroids, dtype=F32)])


def assign(scores, gate, rules=frozenset()):
    """scores [nlist, N] -> list per row, -1 outside the gate."""
    nlist, n = scores.shape
    ids = np.arange(nlist, dtype=np.uint64)[:, None]
    if "ties_high" in rules:
        keys = (score_ord(scores) << np.uint64(32)) | ids
    else:
        keys = (score_ord(scores) << np.uint64(32)) | (np.uint64(0xFFFFFFFF) - ids)
    best = np.argmax(keys, axis=0).astype(np.int64)
    best[~np.asarray(gate, dtype=bool)] = -1
    if "first_launch" in rules:
        best[LAUNCH_ROWS:] = -1
    return best


def make_lists(assignment, nlist):
    """-> offsets [nlist + 1] u64, rows u32: ascending inside a list (a stable sort of ascending rows by list)."""
    member = np.nonzero(assignment >= 0)[0]
    order = np.argsort(assignment[member], kind="stable")
    rows = member[order].astype(np.uint32)
    counts = np.bincount(assignment[member], minlength=nlist).astype(np.uint64)
    return np.concatenate([[np.uint64(0)], np.cumsum(counts, dtype=np.uint64)]).astype(np.uint64), rows


def list_mean_norm2(wide, members, rules=frozenset()):
    """The f64 mean of a list's members (ascending rows) and its squared norm, both sums sequential."""
    vals = wide[members].astype(np.float64)
    with np.errstate(all="ignore"):
        # cumsum: sequential, in row order; np.sum is pairwise along a contiguous axis
        s = np.ascontiguousarray(vals.T).sum(axis=1) if "pairwise_sum" in rules else np.cumsum(vals, axis=0)[-1]
        mean = s / np.float64(members.size)
        return mean, np.cumsum(mean * mean)[-1]                                            # sequential over ascending d


def update(wide, assignment, centroids, rules=frozenset(), reseed=None):
    out = np.array(centroids, dtype=F32, copy=True)
    for l in range(out.shape[0]):
        members = np.nonzero(assignment == l)[0]   # ascending
        if members.size == 0:
            if "reseed_empty" in rules:
                out[l] = reseed
            continue
        mean, norm2 = list_mean_norm2(wide, members, rules)
        with np.errstate(all="ignore"):
            if "no_normalise" in rules:
                out[l] = mean.astype(F32)
            elif np.isfinite(norm2) and norm2 > 0.0:
                out[l] = (mean / np.sqrt(norm2)).astype(F32)
    return out


class Index:
    def __init__(self, centroids, offsets, rows, live, hreduce, trained, changed_last):
        self.centroids, self.offsets, self.rows, self.live, self.hreduce = centroids, offsets, rows, live, hreduce
        self.trained, self.changed_last = trained, changed_last

    def list_rows(self, l):
        return self.rows[int(self.offsets[l]):int(self.offsets[l + 1])]


def build(oracle, slab_u16, nlist, iters, n_train=0, live=None, init=None, hreduce=0, rules=frozenset()):
    slab_u16 = np.ascontiguousarray(slab_u16, dtype=np.uint16)
    n = slab_u16.shape[0]
    live_b = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    train = training_rows(n, n_train, live_b)
    assert 1 <= nlist <= len(train)
    wide = widen(slab_u16)
    cent = strided_init(slab_u16, train, nlist) if init is None else np.array(init, dtype=F32, copy=True)
    gate = np.zeros(n, dtype=bool)
    gate[train] = True
    prev, changed = None, 0
    for _ in range(iters):
        a = assign(centroid_scores(oracle, slab_u16, cent, hreduce), gate, rules)
        changed = int(gate.sum()) if prev is None else int((a[gate] != prev[gate]).sum())
        prev = a
        cent = update(wide, a, cent, rules, reseed=wide[train[0]])
    final = assign(centroid_scores(oracle, slab_u16, cent, hreduce), live_b, rules)
    offsets, rows = make_lists(final, nlist)
    return Index(cent, offsets, rows, live_b.copy(), hreduce, len(train), changed)


def probe(oracle, index, query, nprobe):
    """The nprobe best centroids: what an F32 index over the centroid matrix answers."""
    lists, _ = oracle.search_top_k_f32(index.centroids, query, nprobe, hreduce=index.hreduce)
    assert lists.size == nprobe
    return lists


def search(oracle, slab_u16, index, query, k, nprobe, live_now=None, row_base=0, rules=frozenset(), row_scores=None, exact=None):
    """-> (global rows, scores, flag).  row_scores: the query's exact score of every row, when the caller has it already;
    exact(query, k, live) -> (rows, scores): the exact search, when the caller has a cheaper one than the oracle's."""
    n = slab_u16.shape[0]
    live = index.live if (live_now is None or "dead_at_build" in rules) else np.asarray(live_now, dtype=bool)
    true_live = index.live if live_now is None else np.asarray(live_now, dtype=bool)
    lists = probe(oracle, index, query, nprobe)
    if "stop_at_empty" in rules:
        empty = [i for i, l in enumerate(lists) if index.list_rows(int(l)).size == 0]
        lists = lists[:empty[0]] if empty else lists
    cand = np.concatenate([index.list_rows(int(l)) for l in lists]) if len(lists) else np.zeros(0, np.uint32)
    cand = cand[live[cand]].astype(np.uint32)
    sc = row_scores[cand] if row_scores is not None else oracle.gather_dot(slab_u16, query, cand, index.hreduce)
    if "stride_k_tiles" in rules and k < TILE_ROWS:
        # the table of the query's slots: per probed list its best k, best first, in a row of TILE_ROWS entries; read k apart
        table = np.full((len(lists), TILE_ROWS), -1, dtype=np.int64)   # positions in cand; -1: no entry
        at = 0
        for j, l in enumerate(lists):
            n = int(live[index.list_rows(int(l))].sum())
            mine = np.arange(at, at + n)
            best = mine[np.argsort(order_keys(sc[mine], cand[mine]), kind="stable")[::-1][:k]]
            table[j, :best.size] = best
            at += n
        read = np.concatenate([table.ravel()[j * k:j * k + k] for j in range(len(lists))]) if len(lists) else np.zeros(0, np.int64)
        read = read[read >= 0]
        cand, sc = cand[read], np.asarray(sc, dtype=F32)[read]
    order = np.argsort(order_keys(sc, cand), kind="stable")[::-1][:k]
    rows, scores = cand[order], np.asarray(sc, dtype=F32)[order]
    need = min(k, int(true_live.sum()))
    if rows.size < need:
        flag = EMPTY if rows.size == 0 else UNDERFILLED
        if exact is not None:
            rows, scores = exact(query, k, true_live)
        else:
            rows, scores = oracle.search_top_k(slab_u16, query, k, live=true_live, hreduce=index.hreduce)
        return rows.astype(np.uint32) + np.uint32(row_base), scores, flag
    return rows + np.uint32(row_base), scores, APPROXIMATE


def rows_scored(oracle, index, query, nprobe):
    return int(sum(len(index.list_rows(int(l))) for l in probe(oracle, index, query, nprobe)))


def certify_nprobe(candidates, answer, exact_rows, target, alpha):
    """fsgpu_ivf_certify_nprobe restated: answer(nprobe) -> [(rows, flag)] per query; exact_rows[q] the exact top-k.
    -> ((nprobe, bound, meets), sweep)"""
    def measure(p):
        return [ann_ref.recall_sample(rows, flag, exact_rows[q]) for q, (rows, flag) in enumerate(answer(p))]
    return ann_ref.calibrate(candidates, measure, target, alpha)

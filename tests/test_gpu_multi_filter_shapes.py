"""The gather scan of a per-query-filtered batch (filter_gather_kernels.hip, vector_index_filtered.cpp) at the dimensions, k and scores
that test_gpu_multi_filter.py's two dimensions never reach: no group of four chunks, leftover chunks, every row pitch from 64 to 2,112
bytes, the largest dimension of both k tiers and the first one refused, blocks that carry a list across tiles at the new shapes,
ties across a tile boundary and the k-th place, non-finite scores.  Cases: tests/multi_filter_cases.py.

The contract is test_gpu_multi_filter.py's: per query the rows, f32 score bits and count of search_batch(q, k, allow=mask, exact=True)
AND of oracle.search_top_k(slab, q, k, live=live & mask) — and the PATH, read from the handle's counters: a refused shape would answer
just as correctly through the per-query search, so every case asserts where its queries were counted."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import multi_filter_cases as M  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}   # per case: slab, queries, index, filters — made once, never changed


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    assert fa_mod._lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    return fa_mod


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def indexed(fa, key, make):
    if key not in _cache:
        c = make()
        idx = fa.VectorIndex.from_slab(c["slab"], device=0)
        c["filters"] = [idx.resident_filter(m) for m in c["masks"]]     # made while every row is live ...
        idx.set_live(c["live"])                                          # ... the tombstones come afterwards
        c["idx"] = idx
        _cache[key] = c
    return _cache[key]


def same_scores(got, want):
    """NaN where the reference has a NaN (payload and sign are the platform's), the reference's bits everywhere else."""
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and np.array_equal(bits(got[~nan]), bits(want[~nan])))


def run(c, oracle, k, gathered, what):
    """One call over all of the case's queries; every query's answer against the oracle and the index's exact search; the counters:
    all queries counted by the gather scan (gathered) or all by the per-query search."""
    idx, fq, q = c["idx"], c["fq"], c["queries"]
    before = idx.multi_filter_stats()
    rows, scores, counts, fb = idx.search_batched_per_query_filters(q, k, c["filters"], fq)
    after = idx.multi_filter_stats()
    moved = (after.gathered - before.gathered, after.fallbacks - before.fallbacks, after.scanned - before.scanned,
             after.unfiltered - before.unfiltered)
    print(f"{what}: k {k}: {fq.size} queries, gathered {moved[0]}, per-query {moved[1]}, reported fallbacks {fb}")
    assert moved == ((fq.size, 0, 0, 0) if gathered else (0, fq.size, 0, 0)), (what, moved)
    assert fb == (0 if gathered else fq.size)
    for f in sorted(set(int(v) for v in fq)):
        members = np.flatnonzero(fq == f)
        er, es, ec = idx.search_batch(q[members], k, allow=c["masks"][f], exact=True)
        for j, i in enumerate(members):
            wr, ws = oracle.search_top_k(c["slab"], q[i], k, live=c["live"] & c["masks"][f])
            n = int(counts[i])
            assert n == len(wr) == int(ec[j]) == min(k, int((c["live"] & c["masks"][f]).sum())), (what, i, n, len(wr), int(ec[j]))
            assert np.array_equal(rows[i, :n], wr) and same_scores(scores[i, :n], ws), (what, "oracle", i)
            assert np.array_equal(er[j, :n], wr) and same_scores(es[j, :n], ws), (what, "exact search", i)
    return rows, scores, counts


# ---- a. dimensions and k -----------------------------------------------------------------------------------------------------------------

def test_the_planner_takes_what_the_lds_formula_allows():
    assert M.gather_supported(M.MAX_DIM_K64, 64) and not M.gather_supported(M.MAX_DIM_K64 + 8, 64) and not M.gather_supported(M.MAX_DIM_K64, 65)
    assert M.gather_supported(M.MAX_DIM_K256, 256) and not M.gather_supported(M.MAX_DIM_K256 + 8, 65)
    assert not any(M.gather_supported(d, k) for d, k in M.REFUSED)
    assert len(M.SHAPES) == len(M.DIMS) * len(M.KS) - 2      # all but the larger limit at k 65 and 256


@pytest.mark.parametrize("dim,k", M.SHAPES)
def test_every_supported_shape_is_gathered_and_exact(fa, oracle, dim, k):
    c = indexed(fa, ("shape", dim), lambda: M.shape_case(oracle, dim))
    allowed = [int(m.sum()) for m in c["masks"]]
    assert all(0 < a * 50 < M.N for a in allowed) and max(M.GROUP_SIZES) > 4
    run(c, oracle, k, True, f"dim {dim} (groups, leftover) {M.DIMS[dim]} pitch {M.row_pitch(dim)}")


# ---- b. blocks that walk several tiles ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [40, 200])
@pytest.mark.parametrize("k", [10, 64, 256])
def test_blocks_walk_several_tiles_at_the_new_shapes(fa, oracle, dim, k):
    """128 selective filters: the planner gives each group 8 blocks (about four per CU over all groups, at least 8 a group), and 700
    rows are 11 tiles, so blocks 0 - 2 of every group walk two tiles — the k <= 64 form parks its one-entry-per-lane list between
    them, the k <= 256 form reloads its list.  Three queries for the first ten groups, one for the rest."""
    nf = 128
    n = 40_000

    def make():
        rng = np.random.default_rng(41 + dim)
        masks = []
        for _ in range(nf):
            m = np.zeros(n, dtype=bool)
            m[rng.choice(n, 700, replace=False)] = True        # 700 x 50 < 40,000: selective
            masks.append(m)
        live = np.ones(n, dtype=bool)
        live[rng.choice(n, 4_000, replace=False)] = False
        fq = np.concatenate([np.arange(nf), np.arange(10), np.arange(10)]).astype(np.int32)
        queries = np.stack([oracle.clustered_query(i, dim) for i in range(fq.size)]).astype(np.float32)
        return dict(slab=oracle.clustered_corpus_f16(0, n, dim), masks=masks, live=live, fq=fq, queries=queries)
    c = indexed(fa, ("tiles", dim), make)
    assert -(-700 // M.TILE_ROWS) == 11
    run(c, oracle, k, True, f"several tiles, dim {dim}")


# ---- c. refused shapes take the per-query path --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,k", M.REFUSED)
def test_the_first_refused_shapes_are_answered_query_by_query(fa, oracle, dim, k):
    """One dimension step past each tier's limit, the k <= 64 limit at k = 65, and a dimension that is no multiple of 8: the same
    answers, counted as per-query fallbacks and not as gathered."""
    c = indexed(fa, ("shape", dim), lambda: M.shape_case(oracle, dim))
    run(c, oracle, k, False, f"refused: dim {dim}")
    if M.gather_supported(dim, 64):    # the very same index and filters are gathered again at a k of the other tier
        run(c, oracle, 64, True, f"dim {dim} at k 64")


# ---- d. ties and non-finite scores ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [40, 384])
@pytest.mark.parametrize("k", M.TIE_KS)
def test_ties_across_a_tile_boundary_and_non_finite_scores(fa, oracle, dim, k):
    c = indexed(fa, ("ties", dim), lambda: M.tie_case(oracle, dim))
    rows, scores, counts = run(c, oracle, k, True, f"ties and non-finite scores, dim {dim}")
    nq = c["fq"].size // 2
    for f, at in ((0, 10), (1, 70)):
        got = rows[f * nq, :counts[f * nq]]
        inside = np.isin(c["dups"][f], got)
        if k == at:        # the equal rows straddle the k-th place: the lower rows are in, the higher ones out
            assert 0 < inside.sum() < inside.size and not (np.diff(inside.astype(int)) > 0).any(), (f, inside)
        if inside.sum() > 1:   # equal bits, row ascending
            pos = [int(np.flatnonzero(got == r)[0]) for r in c["dups"][f][inside]]
            assert pos == sorted(pos) and np.unique(bits(scores[f * nq, pos])).size == 1
    if k == 256:           # the whole list comes back: +inf in front, -inf and NaN (one rank: row ascending) at the end
        for i in range(c["fq"].size):
            s = scores[i, :counts[i]]
            assert np.isnan(s).any() and (np.isinf(s).any() or i % nq >= 6)

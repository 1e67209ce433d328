"""A filter per query in one batched call (filter_gather_kernels.hip, vector_index_filtered.cpp).

The contract: per query, the rows, f32 score bits and count of the exact search with that query's bitmap — checked against
search_batch(q, k, allow=mask, exact=True) of the same index AND oracle.search_top_k(slab, q, k, live=live & mask) — and the PATH:
the queries of selective filters are counted by the gather scan, none falls back.  Every shape here is F16, dim % 8 == 0, k <= 256:
inside the gather scan's coverage, so `fallbacks == 0` is a condition of the test, not a tolerance.  Fixture: tests/multi_filter_ref.py.
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import multi_filter_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
_cache = {}   # per dimension: slab, queries, index, filters, references — computed once, never changed


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    assert fa_mod._lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    return fa_mod


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def case(fa, oracle, dim):
    if dim not in _cache:
        slab = R.doctor_slab(oracle.clustered_corpus_f16(0, R.N, dim))
        queries = np.stack([oracle.clustered_query(q, dim) for q in range(R.NQ)])
        masks = R.filter_masks()
        idx = fa.VectorIndex.from_slab(slab, device=0)
        filters = [idx.resident_filter(m) for m in masks]      # made while every row is live ...
        live = R.tombstones(masks)
        idx.set_live(live)                                      # ... the tombstones come afterwards
        _cache[dim] = dict(slab=slab, queries=queries, masks=masks, idx=idx, filters=filters, live=live, fq=R.assignment(), want={})
    return _cache[dim]


def reference(c, oracle, k):
    """Per query (rows, scores) of the oracle, and of the index's own exact search filter group by filter group."""
    if k not in c["want"]:
        fq, q, idx = c["fq"], c["queries"], c["idx"]
        orc = []
        for i in range(R.NQ):
            live = c["live"] if fq[i] < 0 else c["live"] & c["masks"][fq[i]]
            orc.append(oracle.search_top_k(c["slab"], q[i], k, live=live))
        own = [None] * R.NQ
        for f in sorted(set(int(v) for v in fq)):
            members = np.flatnonzero(fq == f)
            er, es, ec = idx.search_batch(q[members], k, allow=None if f < 0 else c["masks"][f], exact=True)
            for j, i in enumerate(members):
                own[i] = (er[j, : ec[j]].copy(), es[j, : ec[j]].copy())
        c["want"][k] = (orc, own)
    return c["want"][k]


def assert_answers(got, want, queries=None, what=""):
    rows, scores, counts = got[:3]
    orc, own = want
    for j in range(rows.shape[0]):
        i = j if queries is None else int(queries[j])
        for name, (wr, ws) in (("oracle", orc[i]), ("exact search", own[i])):
            n = int(counts[j])
            assert n == len(wr), (what, name, i, n, len(wr))
            assert np.array_equal(rows[j, :n], wr) and np.array_equal(bits(scores[j, :n]), bits(ws)), (what, name, i)


# ---- 1. the row list, built on the device ----------------------------------------------------------------------------------------

def test_row_list_equals_flatnonzero(fa, oracle):
    n, dim = 4_099, 64                       # 64 words + a tail word of 3 bits
    slab = oracle.clustered_corpus_f16(0, n, dim)
    idx = fa.VectorIndex.from_slab(slab, device=0)
    rng = np.random.default_rng(3)
    masks = []
    for count in (0, 1, 63, 64, 65, 81):
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, count, replace=False)] = True
        masks.append(m)
    ends = np.zeros(n, dtype=bool)
    ends[[0, n - 1]] = True                  # the first row and the last
    masks.append(ends)
    run = np.zeros(n, dtype=bool)
    run[4_030:] = True                       # whole words and the whole tail
    run[0] = True
    masks.append(run)
    masks.append(np.ones(n, dtype=bool))
    for m in masks:
        f = idx.resident_filter(m)
        assert np.array_equal(f.rows(), np.flatnonzero(m).astype(np.uint32)), int(m.sum())
        assert np.array_equal(f.rows(), np.flatnonzero(m).astype(np.uint32))     # the cached list
    # garbage bits past N in the tail word are not rows
    from frankensearch_amd.index import pack_bitmap
    for m in masks[:7]:
        words = pack_bitmap(m)
        words[-1] |= np.uint64(0xFFFFFFFFFFFFFFFF) << np.uint64(n & 63)
        f = idx.resident_filter(words)
        assert f.allowed_rows() == int(m.sum())
        assert np.array_equal(f.rows(), np.flatnonzero(m).astype(np.uint32))


# ---- 2. the gather scan: same bits as the exact search and the oracle, and the path ran -------------------------------------------

@pytest.mark.parametrize("dim", [64, 384])
@pytest.mark.parametrize("k", [1, 10, 256])
def test_mixed_batch_equals_exact_search_and_oracle(fa, oracle, dim, k):
    c = case(fa, oracle, dim)
    idx, fq = c["idx"], c["fq"]
    want = reference(c, oracle, k)
    before = idx.multi_filter_stats()
    got = idx.search_batched_per_query_filters(c["queries"], k, c["filters"], fq)
    after = idx.multi_filter_stats()
    assert_answers(got, want, what=(dim, k))
    allowed = np.array([int(m.sum()) for m in c["masks"]])
    selective = int(sum(1 for f in fq if f >= 0 and 0 < allowed[f] * 50 < R.N))
    dense = int(np.sum(fq == R.DENSE_FILTER))
    assert selective == R.NQ - 19 - 11 - 3
    assert after.gathered - before.gathered == selective                 # the gather scan answered exactly the selective queries
    assert after.fallbacks - before.fallbacks == 0
    assert after.scanned - before.scanned == dense and after.unfiltered - before.unfiltered == 19
    counts = got[2]
    assert np.all(counts[fq == R.EMPTY_FILTER] == 0)
    if k > 1:   # a filter with fewer live allowed rows than k answers with all of them
        short = [i for i in range(R.NQ) if fq[i] >= 0 and 0 < allowed[fq[i]] < k]
        assert short and all(0 < counts[i] < k for i in short if allowed[fq[i]] > 1)
    if k >= 10 and dim == 384:   # the duplicated rows tie on the score and come out row-ascending
        hit = [i for i in range(R.NQ) if 100 in got[0][i, : counts[i]] and 5_000 in got[0][i, : counts[i]]]
        for i in hit:
            r = got[0][i, : counts[i]].tolist()
            assert r.index(100) < r.index(5_000) and bits(got[1][i])[r.index(100)] == bits(got[1][i])[r.index(5_000)]


def test_selective_groups_alone_report_no_fallback(fa, oracle):
    c = case(fa, oracle, 64)
    allowed = np.array([int(m.sum()) for m in c["masks"]])
    pick = np.array([i for i in range(R.NQ) if c["fq"][i] >= 0 and allowed[c["fq"][i]] * 50 < R.N])   # selective and empty filters
    got = c["idx"].search_batched_per_query_filters(c["queries"][pick], 10, c["filters"], c["fq"][pick])
    assert got[3] == 0
    assert_answers(got, reference(c, oracle, 10), queries=pick)


def test_a_list_longer_than_its_blocks_hold_in_one_tile(fa, oracle):
    """At k = 256 a group gets at most 64 blocks (64 lists x 256 entries fill the merge's one-pass form), so a list of more than
    64 x 64 rows makes blocks walk several tiles and carry a query's list from one tile to the next — the one path the 20,000-row
    fixture cannot reach (a selective filter there has fewer than 400 rows).  5,000 of 262,181 rows: 79 tiles on 64 blocks."""
    n, dim, k = 262_181, 64, 256
    slab = oracle.clustered_corpus_f16(0, n, dim)
    rng = np.random.default_rng(31)
    mask = np.zeros(n, dtype=bool)
    mask[rng.choice(n, 5_000, replace=False)] = True
    mask[[0, n - 1]] = True
    small = np.zeros(n, dtype=bool)
    small[rng.choice(n, 300, replace=False)] = True
    idx = fa.VectorIndex.from_slab(slab, device=0)
    filters = [idx.resident_filter(mask), idx.resident_filter(small)]
    live = np.ones(n, dtype=bool)
    live[rng.choice(np.flatnonzero(mask), 400, replace=False)] = False
    idx.set_live(live)
    q = np.stack([oracle.clustered_query(i, dim) for i in range(9)])
    fq = np.array([0, 1, 0, 0, 1, 0, 0, 0, 0], dtype=np.int32)
    before = idx.multi_filter_stats()
    rows, scores, counts, fb = idx.search_batched_per_query_filters(q, k, filters, fq)
    after = idx.multi_filter_stats()
    assert fb == 0 and after.gathered - before.gathered == 9 and after.fallbacks == before.fallbacks
    for i in range(9):
        m = mask if fq[i] == 0 else small
        wr, ws = oracle.search_top_k(slab, q[i], k, live=live & m)
        assert int(counts[i]) == len(wr) == k
        assert np.array_equal(rows[i], wr) and np.array_equal(bits(scores[i]), bits(ws)), i
    er, es, ec = idx.search_batch(q[fq == 0], k, allow=mask, exact=True)
    assert np.array_equal(er, rows[fq == 0]) and np.array_equal(bits(es), bits(scores[fq == 0])) and np.array_equal(ec, counts[fq == 0])


@pytest.mark.parametrize("k", [10, 64])
def test_many_groups_share_the_device_and_walk_several_tiles(fa, oracle, k):
    """For k <= 64 a block keeps a query's k best one per lane and parks them in memory between tiles.  The blocks of a call are
    shared out over its groups (about four per CU in all, at least 8 per group): 128 groups of 600 rows get 8 blocks for 10 tiles
    each on a 256-CU device, so every block walks more than one tile.  Three queries per group for the first groups, one for the rest."""
    n, dim, nf = 40_000, 64, 128
    slab = oracle.clustered_corpus_f16(0, n, dim)
    rng = np.random.default_rng(41)
    masks = []
    for f in range(nf):
        m = np.zeros(n, dtype=bool)
        m[rng.choice(n, 600, replace=False)] = True       # 600 x 50 < 40,000: selective
        masks.append(m)
    idx = fa.VectorIndex.from_slab(slab, device=0)
    filters = [idx.resident_filter(m) for m in masks]
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, 4_000, replace=False)] = False
    idx.set_live(live)
    fq = np.concatenate([np.arange(nf), np.arange(10), np.arange(10)]).astype(np.int32)
    q = np.stack([oracle.clustered_query(i, dim) for i in range(fq.size)])
    before = idx.multi_filter_stats()
    rows, scores, counts, fb = idx.search_batched_per_query_filters(q, k, filters, fq)
    after = idx.multi_filter_stats()
    assert fb == 0 and after.gathered - before.gathered == fq.size and after.fallbacks == before.fallbacks
    for i in range(fq.size):
        wr, ws = oracle.search_top_k(slab, q[i], k, live=live & masks[fq[i]])
        assert int(counts[i]) == len(wr) == k
        assert np.array_equal(rows[i], wr) and np.array_equal(bits(scores[i]), bits(ws)), i


# ---- 3. invariance ------------------------------------------------------------------------------------------------------------------

def test_permuted_order_and_each_query_alone_give_the_same_bits(fa, oracle):
    c = case(fa, oracle, 64)
    idx, k = c["idx"], 10
    want = reference(c, oracle, k)
    perm = np.random.default_rng(21).permutation(R.NQ)
    got = idx.search_batched_per_query_filters(c["queries"][perm], k, c["filters"], c["fq"][perm])
    assert_answers(got, want, queries=perm, what="permuted")
    for i in range(R.NQ):
        one = idx.search_batched_per_query_filters(c["queries"][i], k, c["filters"], c["fq"][i: i + 1])
        assert_answers(one, want, queries=[i], what="alone")


# ---- 4. errors: refused before anything is launched -----------------------------------------------------------------------------------

def test_bad_arguments_are_refused_with_no_launch(fa, oracle):
    c = case(fa, oracle, 64)
    idx, q, filters = c["idx"], c["queries"][:4], c["filters"]
    before = idx.multi_filter_stats()
    with pytest.raises(fa.InvalidConfig):
        idx.search_batched_per_query_filters(q, 10, filters, [0, 1, len(filters), 2])
    with pytest.raises(fa.InvalidConfig):
        idx.search_batched_per_query_filters(q, 10, filters, [0, -2, 1, 2])
    with pytest.raises(fa.DimensionMismatch):
        idx.search_batched_per_query_filters(np.zeros((4, 72), np.float32), 10, filters, [0, 1, 2, 3])
    # a filter of another index
    other_slab = oracle.clustered_corpus_f16(0, 3_000, 64)
    other = fa.VectorIndex.from_slab(other_slab, device=0)
    stranger = other.resident_filter(np.ones(3_000, dtype=bool))
    with pytest.raises(fa.InvalidConfig):
        idx.search_batched_per_query_filters(q, 10, filters[:3] + [stranger], [0, 1, 2, -1])   # refused even when no query names it
    # a filter made before a vacuum
    live = np.ones(3_000, dtype=bool)
    live[::3] = False
    old = other.resident_filter(np.ones(3_000, dtype=bool))
    other.set_live(live)
    other.vacuum()
    with pytest.raises(fa.InvalidConfig):
        other.search_batched_per_query_filters(q, 10, [old], [0, 0, 0, 0])
    fresh = other.resident_filter(np.arange(other.record_count()) % 100 == 0)
    rows, scores, counts, fb = other.search_batched_per_query_filters(q, 10, [fresh], [0, 0, 0, 0])
    assert np.all(counts == 10) and np.all(rows % 100 == 0) and fb == 0
    assert idx.multi_filter_stats() == before
    # k == 0: counts of 0, as search_top_k
    assert np.all(idx.search_batched_per_query_filters(q, 0, filters, [0, 1, -1, 35])[2] == 0)


# ---- 5. the device-queries form -------------------------------------------------------------------------------------------------------

def test_device_queries_form_gives_the_host_form_answers(fa, oracle):
    import torch
    c = case(fa, oracle, 384)
    idx, k = c["idx"], 10
    host = idx.search_batched_per_query_filters(c["queries"], k, c["filters"], c["fq"])
    dev = torch.device("cuda:0")
    q = torch.from_numpy(c["queries"]).to(dev)
    rows = torch.full((R.NQ, k), -1, dtype=torch.int32, device=dev)
    scores = torch.zeros((R.NQ, k), dtype=torch.float32, device=dev)
    counts = torch.zeros(R.NQ, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    stream = torch.cuda.current_stream(dev).cuda_stream
    idx.search_batched_per_query_filters(None, k, c["filters"], c["fq"], queries_ptr=q.data_ptr(), nq=R.NQ,
                                         out_ptrs=(rows.data_ptr(), scores.data_ptr(), counts.data_ptr()), stream=stream)
    torch.cuda.synchronize()
    got = (rows.cpu().numpy().view(np.uint32), scores.cpu().numpy(), counts.cpu().numpy().view(np.uint32))
    assert np.array_equal(got[2], host[2])
    assert_answers(got, reference(c, oracle, k), what="device form")
    for i in range(R.NQ):
        n = int(host[2][i])
        assert np.array_equal(got[0][i, :n], host[0][i, :n]) and np.array_equal(bits(got[1][i, :n]), bits(host[1][i, :n]))

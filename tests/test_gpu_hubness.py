"""GPU checks of the query-hubness table build (hubness_kernels.hip) and of the searcher's phase-1 correction, all through the C ABI.
The device table equals fsgpu_query_hubness on the rows fetched from the slab bit for bit, for EVERY row — no tolerance, no sample
of rows; the selected top-k multiset equals tests/hubness_ref.py's and, for dim % 32 == 0, the scan's own score bits."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hubness_ref as H  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_values(a, b):
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))))


def _fetch(idx):
    return np.stack([idx.vector_at(r) for r in range(idx.record_count())])


def _f16_index(fa, rng, n, dim, live=None):
    vec = H.unit_rows(rng, n, dim).astype(np.float16)
    return fa.VectorIndex.from_slab(vec, live=live), vec.astype(F32)


def _f32_index(fa, rng, n, dim, tmp_path, name):
    """An F32 slab of wide-range values (where a wrong add order shows): rows scaled over six decades."""
    vec = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-7, 7, (n, 1))) * np.exp(rng.uniform(-2, 2, (n, dim)))).astype(F32)
    ids = [f"doc-{i:05d}" for i in range(n)]
    path = str(tmp_path / name)
    fa.write_fsvi(path, list(zip(ids, vec)), quantization=0)
    return fa.VectorIndex.open(path)


def _check(fa, idx, queries, kq, mode=H.HREDUCE_SSE2, rows=None):
    """device table == fsgpu_query_hubness on the fetched rows, every row, bit for bit"""
    idx.set_hreduce(mode)
    got = idx.compute_query_hubness(queries, kq)
    rows = _fetch(idx) if rows is None else rows
    want = fa.compute_query_hubness(rows, queries, kq, hreduce=mode)
    diff = np.flatnonzero(~((bits(got) == bits(want)) | ((got == 0) & (want == 0))))
    print(f"rows {rows.shape[0]} x dim {rows.shape[1]}, Q {len(queries)}, kq {kq}, hreduce {mode}: rows differing {diff.size}")
    assert got.shape == (rows.shape[0],)
    assert diff.size == 0, (diff[:8], got[diff[:8]], want[diff[:8]])
    return got, rows


@pytest.mark.parametrize("dim", [256, 384])
def test_f16_slab_20000_rows_by_1000_queries_equals_the_host_restatement_for_every_row(dim):
    fa = _fa()
    rng = np.random.default_rng(dim)
    idx, vec = _f16_index(fa, rng, 20_000, dim)
    queries = H.unit_rows(rng, 1000, dim)
    rows = _fetch(idx)
    assert np.array_equal(bits(rows), bits(vec))   # widening an f16 row is exact
    got, _ = _check(fa, idx, queries, 10, rows=rows)
    assert np.isfinite(got).all() and got.min() > 0
    for kq in (1, 64):
        _check(fa, idx, queries, kq, rows=rows)
    for mode in (H.HREDUCE_AVX, H.HREDUCE_SEQ):
        _check(fa, idx, queries[:333], 10, mode, rows=rows)
    idx.close()


@pytest.mark.parametrize("dim,n", [(4, 3001), (43, 2500), (100, 2500), (768, 1203), (1024, 300)])
def test_general_dimensions_query_counts_and_row_counts_off_the_tile(dim, n):
    fa = _fa()
    rng = np.random.default_rng(1000 + dim)
    live = np.ones(n, dtype=bool)
    live[n // 3] = False   # a tombstoned row still gets its value: the table is indexed by VectorHit::index
    idx, vec = _f16_index(fa, rng, n, dim, live=fa.pack_bitmap(live))
    rows = _fetch(idx)
    queries = H.unit_rows(rng, 203, dim)
    for mode in (H.HREDUCE_SSE2, H.HREDUCE_AVX, H.HREDUCE_SEQ):
        got, _ = _check(fa, idx, queries, 10, mode, rows=rows)
        # ... and the numpy restatement, whose dot is checked against the oracle on the CPU
        assert same_values(got, H.compute_query_hubness(rows, queries, 10, mode))
    for nq, kq in ((1, 10), (7, 10), (7, 7), (16, 1), (17, 64), (203, 64), (203, 65), (203, 300)):
        # Q = 1; k clamps to Q = 7; Q off the kernel's chunk of 16; k = 65 and k = 203 run the host restatement on fetched blocks
        _check(fa, idx, queries[:nq], kq, rows=rows)
    assert idx.compute_query_hubness(queries[:0], 10).tolist() == [0.0] * n
    assert idx.compute_query_hubness(queries, 0).tolist() == [0.0] * n
    idx.close()


@pytest.mark.parametrize("dim", [100, 384])
def test_f32_slab_of_wide_range_values(dim, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(2000 + dim)
    idx = _f32_index(fa, rng, 3001, dim, tmp_path, f"wide{dim}.fsvi")
    queries = (rng.standard_normal((150, dim)) * np.exp(rng.uniform(-3, 3, (150, 1)))).astype(F32)
    rows = _fetch(idx)
    for mode in (H.HREDUCE_SSE2, H.HREDUCE_AVX, H.HREDUCE_SEQ):
        got, _ = _check(fa, idx, queries, 10, mode, rows=rows)
        assert same_values(got, H.compute_query_hubness(rows, queries, 10, mode))
    for kq in (1, 64, 65):
        _check(fa, idx, queries, kq, rows=rows)
    idx.close()


def test_batch_independence_and_the_sharded_handle():
    fa = _fa()
    rng = np.random.default_rng(31)
    n, dim = 10_006, 256
    vec = H.unit_rows(rng, n, dim).astype(np.float16)
    queries = H.unit_rows(rng, 300, dim)
    whole = fa.VectorIndex.from_slab(vec)
    table = whole.compute_query_hubness(queries, 10)
    lo, hi = fa.VectorIndex.from_slab(vec[:n // 2]), fa.VectorIndex.from_slab(vec[n // 2:])
    halves = np.concatenate([lo.compute_query_hubness(queries, 10), hi.compute_query_hubness(queries, 10)])
    assert np.array_equal(bits(table), bits(halves))
    P = fa.NativeShardedIndex.EXCHANGE_PEER_COPY
    for groups, row_shards in ((1, 1), (1, 2), (2, 2), (3, 1)):
        sh = fa.NativeShardedIndex.from_slab(vec, [0] * (groups * row_shards), exchange=P, query_groups=groups)
        got = sh.compute_query_hubness(queries, 10)
        assert np.array_equal(bits(got), bits(table)), (groups, row_shards)
        with pytest.raises(fa.DimensionMismatch):
            sh.compute_query_hubness(queries[:, :100], 10)
        sh.close()
    for h in (whole, lo, hi):
        h.close()


@pytest.mark.parametrize("dim", [256, 384, 43])
def test_the_selected_top_k_equals_the_restatement_and_the_scans_score_bits(dim):
    fa = _fa()
    rng = np.random.default_rng(40 + dim)
    n, nq, k = 1501, 90, 10
    idx, vec = _f16_index(fa, rng, n, dim)
    queries = H.unit_rows(rng, nq, dim)
    for mode in (H.HREDUCE_SSE2, H.HREDUCE_SEQ):
        idx.set_hreduce(mode)
        table, top = idx.compute_query_hubness(queries, k, want_topk=True)
        want_table, want_top = H.compute_query_hubness(vec, queries, k, mode, want_topk=True)
        assert np.array_equal(bits(top), bits(want_top)) and same_values(table, want_table)
        if dim % 32 == 0:
            # every (row, query) score as the scan computes it: fsgpu_search_topk with k = all rows; the f16 byte dot and
            # dot_product_f32_f32 coincide bit for bit when there are neither leftover chunks nor a tail
            rows_, scores_, counts_ = idx.search_batch(queries, n)
            sims = np.zeros((n, nq), F32)
            for q in range(nq):
                assert int(counts_[q]) == n
                sims[rows_[q], q] = scores_[q]
            assert np.array_equal(bits(top), bits(H.select_top(sims, k)))
    idx.close()


def test_errors():
    fa = _fa()
    rng = np.random.default_rng(5)
    idx, _ = _f16_index(fa, rng, 100, 64)
    with pytest.raises(fa.DimensionMismatch):
        idx.compute_query_hubness(H.unit_rows(rng, 5, 32), 10)
    q = H.unit_rows(rng, 5, 64)
    L = fa._lib.lib()
    assert L.fsgpu_index_compute_query_hubness(idx._h, q.ctypes.data, 5, 64, 10, None) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_compute_query_hubness(idx._h, None, 5, 64, 10, np.zeros(100, F32).ctypes.data) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_compute_query_hubness(None, q.ctypes.data, 5, 64, 10, np.zeros(100, F32).ctypes.data) == fa._lib.ERR_NULL_ARGUMENT
    idx.close()


# ---- the searcher ----

def _queries(rng, nq, n, fast_vocab=5000, quality_vocab=3000, lex=30):
    doc = lambda r: f"doc-{int(r):08d}"
    fast = [rng.integers(0, fast_vocab, int(rng.integers(1, 24))).tolist() for _ in range(nq)]
    qual = [[101] + rng.integers(1000, quality_vocab, int(rng.integers(2, 30))).tolist() + [102] for _ in range(nq)]
    lexical = [[(doc(r), float(lex - i)) for i, r in enumerate(rng.choice(n, lex, replace=False))] for _ in range(nq)]
    return fast, qual, lexical


def _pair(fa, rng, n):
    from frankensearch_amd.synthetic import random_bert_weights
    fast_slab = rng.standard_normal((n, 256)).astype(np.float16).view(np.uint16)
    qual_slab = rng.standard_normal((n, 384)).astype(np.float16).view(np.uint16)
    table = rng.standard_normal((5000, 256)).astype(F32)
    return fast_slab, qual_slab, table, random_bert_weights(5, 3000, 384, 2, 512)


def test_searcher_with_a_table_equals_the_host_side_pipeline_and_is_inert_without_one():
    fa = _fa()
    from frankensearch_amd.host import NativeTwoTierSearcher
    from oracle import fusion_oracle

    rng = np.random.default_rng(606)
    n, nq, k = 20_000, 200, 10
    fetch = 3 * k
    fast_slab, qual_slab, table, w = _pair(fa, rng, n)
    fast, qual = fa.VectorIndex.from_slab(fast_slab), fa.VectorIndex.from_slab(qual_slab)
    m2v, bert = fa.Model2VecEmbedder(table), fa.NativeEmbedder(w)
    doc = lambda r: f"doc-{int(r):08d}"
    fq, qq, lex = _queries(rng, nq, n)
    never = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    base = never.search_many(fq, qq, k, lex, chunk=64)
    base_one = [never.search(fq[qi], qq[qi], k, lex[qi])[:2] for qi in range(0, nq, 10)]
    s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    # the table: built on the device from a background sample of the same embedder's vectors; scaled up so that beta = 0.5 moves ranks
    sample = np.stack([m2v.embed_token_ids(t) for t in _queries(rng, 128, n)[0]])
    r_d = fast.compute_query_hubness(sample, 10)
    r_d = (r_d * F32(8.0)).astype(F32)
    # beta = 0, a detached table, an empty table: byte-identical to a searcher that never had the call made
    for tab, beta in ((r_d, 0.0), (None, 0.5), (r_d[:0], 0.5), (r_d, float("nan")), (r_d, -1.0)):
        s.set_hubness(tab, beta)
        got = s.search_many(fq, qq, k, lex, chunk=64)
        assert got[0] == base[0] and got[1] == base[1], beta
        assert [s.search(fq[qi], qq[qi], k, lex[qi])[:2] for qi in range(0, nq, 10)] == base_one
    def pipeline(qi, fvec, qvec, rescored):
        """the existing tier search -> hubness_ref's penalty + cmp_rank sort -> the oracle's RRF / blend / RRF, on given vectors"""
        r_, s_, c_ = fast.search_batch(fvec, fetch)
        raw = [(doc(r_[0, i]), float(s_[0, i]), int(r_[0, i])) for i in range(int(c_[0]))]
        fh = [(d, float(sc), i) for d, sc, i in H.apply_hubness_penalty(raw, r_d, 0.5)]
        want_i = fusion_oracle.rrf_fuse(lex[qi], fh, k)
        if rescored:   # quality_scores_for_hits of the CORRECTED pool, position by position
            scores = qual.gather_dot(qvec, [i for _, _, i in fh])
            blended = fusion_oracle.blend_two_tier_aligned(fh, [float(x) for x in scores], 0.7)
        else:
            r_, s_, c_ = qual.search_batch(qvec, fetch)
            qh = [(doc(r_[0, i]), float(s_[0, i]), int(r_[0, i])) for i in range(int(c_[0]))]
            blended = fusion_oracle.blend_two_tier(fh, qh, 0.7)
            fidx = {d: i for d, _, i in fh}
            blended = [(d, sc, fidx.get(d, 0xFFFFFFFF)) for d, sc, _ in blended]
        return raw, fh, want_i, fusion_oracle.rrf_fuse(lex[qi], blended, k)

    def sbits(hits):
        return [None if h.semantic_score is None else int(bits(h.semantic_score).reshape(-1)[0]) for h in hits]

    def same_list(got, want, what):
        assert [(h.doc_id, h.rrf_score) for h in got] == [(h.doc_id, h.rrf_score) for h in want], what
        assert sbits(got) == sbits(want), what
        if "initial" in what[0]:
            assert [h.semantic_index for h in got] == [h.semantic_index for h in want], what

    s.set_hubness(r_d, 0.5)
    resc = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, quality_pool=1)
    resc.set_hubness(r_d, 0.5)
    # fshost_two_tier_search_many, Retrieved and RescoredFastPool: both lists of every query against the pipeline
    ini, fin, rf, st, fv, qv = s.search_many(fq, qq, k, lex, chunk=64, want_vectors=True)
    got_r = resc.search_many(fq, qq, k, lex, chunk=64, want_vectors=True)
    assert not rf.any() and not got_r[2].any()
    moved = 0
    for qi in range(nq):
        raw, fh, want_i, want_f = pipeline(qi, fv[qi], qv[qi], False)
        moved += [d for d, _, _ in fh] != [d for d, _, _ in raw]
        same_list(ini[qi], want_i, ("many initial", qi))
        same_list(fin[qi], want_f, ("many final", qi))
        _, _, want_i, want_f = pipeline(qi, got_r[4][qi], got_r[5][qi], True)
        same_list(got_r[0][qi], want_i, ("many rescored initial", qi))
        same_list(got_r[1][qi], want_f, ("many rescored final", qi))
    print(f"pools the correction reordered: {moved} of {nq}")
    assert moved >= nq // 2
    assert got_r[0] == ini
    # fshost_two_tier_search, query by query, on that call's own vectors: initial AND refined lists, both pool modes
    one, one_r = {}, {}
    for qi in range(0, nq, 4):
        fvec, qvec = m2v.embed_token_ids(fq[qi]), bert.embed_token_ids(qq[qi])
        i1, f1, _ = s.search(fq[qi], qq[qi], k, lex[qi])
        _, _, want_i, want_f = pipeline(qi, fvec, qvec, False)
        same_list(i1, want_i, ("search initial", qi))
        same_list(f1, want_f, ("search final", qi))
        assert i1 == ini[qi], qi   # phase 0 depends on nothing batched
        i2, f2, _ = resc.search(fq[qi], qq[qi], k, lex[qi])
        _, _, want_i, want_f = pipeline(qi, fvec, qvec, True)
        same_list(i2, want_i, ("search rescored initial", qi))
        same_list(f2, want_f, ("search rescored final", qi))
        one[qi], one_r[qi] = (i1, f1), (i2, f2)
    # the sharded searcher equals the unsharded one, in the many-query and the per-query form
    P = fa.NativeShardedIndex.EXCHANGE_PEER_COPY
    sfast = fa.NativeShardedIndex.from_slab(fast_slab, [0] * 2, exchange=P)
    squal = fa.NativeShardedIndex.from_slab(qual_slab, [0] * 2, exchange=P)
    assert np.array_equal(bits(sfast.compute_query_hubness(sample, 10) * F32(8.0)), bits(r_d))
    for pool, want, want_one in ((0, (ini, fin), one), (1, (got_r[0], got_r[1]), one_r)):
        sh = NativeTwoTierSearcher(sfast, squal, m2v, bert, doc_id_mode=1, quality_pool=pool)
        sh.set_hubness(r_d, 0.5)
        got = sh.search_many(fq, qq, k, lex, chunk=64)
        assert got[0] == want[0] and got[1] == want[1], pool
        for qi in range(0, nq, 20):
            assert tuple(sh.search(fq[qi], qq[qi], k, lex[qi])[:2]) == want_one[qi], (pool, qi)
        sh.close()
    for h in (never, s, resc, sfast, squal, fast, qual, m2v, bert):
        h.close()


def test_a_table_swapped_during_a_search_never_splits_a_search():
    """fshost_two_tier_set_hubness may be called beside searches: a search keeps the table it started with.  A thread attaches and
    detaches the table as fast as it can while search_many runs in RescoredFastPool mode — where the quality scores are stored by
    position in the corrected pool, so a table that changed between the stages would pair them with the wrong documents.  Every call
    must equal, whole, the answer under the table or the answer without it; per-query callers riding the batching engine get an
    initial list that is one of the two."""
    import threading
    fa = _fa()
    from frankensearch_amd.host import NativeTwoTierSearcher

    rng = np.random.default_rng(707)
    n, nq, k = 20_000, 480, 10
    fast_slab, qual_slab, table, w = _pair(fa, rng, n)
    fast, qual = fa.VectorIndex.from_slab(fast_slab), fa.VectorIndex.from_slab(qual_slab)
    m2v, bert = fa.Model2VecEmbedder(table), fa.NativeEmbedder(w)
    fq, qq, lex = _queries(rng, nq, n)
    sample = np.stack([m2v.embed_token_ids(t) for t in _queries(rng, 128, n)[0]])
    r_d = (fast.compute_query_hubness(sample, 10) * F32(8.0)).astype(F32)
    for pool in (1, 0):
        s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, quality_pool=pool)
        without = s.search_many(fq, qq, k, lex, chunk=32)[:2]
        s.set_hubness(r_d, 0.5)
        with_table = s.search_many(fq, qq, k, lex, chunk=32)[:2]
        assert with_table[0] != without[0] and with_table[1] != without[1]
        stop, swaps = threading.Event(), [0]

        def toggle():
            while not stop.is_set():
                s.set_hubness(None if swaps[0] % 2 else r_d, 0.5)
                swaps[0] += 1

        t = threading.Thread(target=toggle)
        t.start()
        try:
            seen = {"with": 0, "without": 0}
            for _ in range(12):
                got = s.search_many(fq, qq, k, lex, chunk=32)[:2]
                which = "with" if got[0] == with_table[0] else "without"
                assert (got[0], got[1]) == ((with_table[0], with_table[1]) if which == "with" else (without[0], without[1])), pool
                seen[which] += 1
            # concurrent per-query callers through the batching engine: a chunk takes its snapshot at admission
            s.set_batching(64, 500)
            bad = []

            def caller(lo):
                for qi in range(lo, nq, 8):
                    i1, f1, _ = s.search(fq[qi], qq[qi], k, lex[qi])
                    if i1 != with_table[0][qi] and i1 != without[0][qi]:
                        bad.append(qi)
            callers = [threading.Thread(target=caller, args=(lo,)) for lo in range(8)]
            for c in callers:
                c.start()
            for c in callers:
                c.join()
            s.set_batching(0, 0)
            assert bad == []
        finally:
            stop.set()
            t.join()
        print(f"pool mode {pool}: {swaps[0]} swaps during 12 calls; calls answered with the table {seen['with']}, without {seen['without']}")
        assert swaps[0] > 100
        s.close()
    for h in (fast, qual, m2v, bert):
        h.close()


def test_a_planted_hub_is_demoted_below_a_specific_row():
    """Every query of the log shares eight tokens, so their embeddings share a direction; the planted row is the log's centroid. It
    is near EVERY query of that distribution (a hub by construction: its r_d is the mean of its ten greatest cosines to the log,
    far above the corpus median), while the specific row holds only the probe's own component."""
    fa = _fa()
    from frankensearch_amd.host import NativeTwoTierSearcher
    from frankensearch_amd.synthetic import random_bert_weights

    rng = np.random.default_rng(909)
    n, k = 5000, 10
    table = rng.standard_normal((5000, 256)).astype(F32)
    m2v = fa.Model2VecEmbedder(table)
    common = rng.choice(5000, 8, replace=False).tolist()
    log = [common + rng.integers(0, 5000, 4).tolist() for _ in range(256)]
    probe_ids = common + rng.integers(0, 5000, 4).tolist()
    unit = lambda v: (v / np.linalg.norm(v)).astype(F32)
    sample = np.stack([unit(m2v.embed_token_ids(t)) for t in log])
    p = unit(m2v.embed_token_ids(probe_ids))
    c = unit(sample.mean(axis=0))
    a = float(p @ c)
    corpus = H.unit_rows(rng, n, 256)
    HUB, SPECIFIC = 1234, 4321
    corpus[HUB] = c
    corpus[SPECIFIC] = unit(p - F32(a) * c)
    fast_slab = corpus.astype(np.float16)
    qual_slab = H.unit_rows(rng, n, 384).astype(np.float16)
    fast, qual = fa.VectorIndex.from_slab(fast_slab), fa.VectorIndex.from_slab(qual_slab)
    bert = fa.NativeEmbedder(random_bert_weights(5, 3000, 384, 2, 512))
    r_d = fast.compute_query_hubness(sample, 10)
    print(f"cos(probe, centroid) = {a:.3f}; r_d: hub {r_d[HUB]:.3f}, specific row {r_d[SPECIFIC]:.3f}, corpus median {np.median(r_d):.3f}, "
          f"corpus max without the hub {np.max(np.delete(r_d, HUB)):.3f}")
    assert r_d[HUB] > 3 * np.median(r_d) and r_d[HUB] == r_d.max()
    s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    quality_ids = [101, 1500, 1600, 102]
    doc = lambda r: f"doc-{int(r):08d}"
    before = [h.doc_id for h in s.search(probe_ids, quality_ids, k, [])[0]]
    s.set_hubness(r_d, 0.5)
    after = [h.doc_id for h in s.search(probe_ids, quality_ids, k, [])[0]]
    print("initial list before:", before[:4], "after:", after[:4])
    assert before[0] == doc(HUB) and doc(SPECIFIC) in before            # the hub leads the uncorrected top-k
    assert before.index(doc(HUB)) < before.index(doc(SPECIFIC))
    assert doc(HUB) in after and after.index(doc(SPECIFIC)) < after.index(doc(HUB))   # the specific row outranks it afterwards
    for h in (s, fast, qual, m2v, bert):
        h.close()

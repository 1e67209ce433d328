"""GPU checks of the searcher's phase-1 neighbour smoothing (fshost_two_tier_set_neighbor_smoothing) over a k-NN graph built by the
device call: Initial and Refined lists against a host pipeline written here — tier answers -> tests/smooth_ref.py -> the library's
RRF and blend."""
import os
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hubness_ref as H  # noqa: E402
import smooth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
doc = lambda r: f"doc-{int(r):08d}"


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _queries(rng, nq, n, fast_vocab=5000, quality_vocab=3000, lex=30):
    fast = [rng.integers(0, fast_vocab, int(rng.integers(1, 24))).tolist() for _ in range(nq)]
    qual = [[101] + rng.integers(1000, quality_vocab, int(rng.integers(2, 30))).tolist() + [102] for _ in range(nq)]
    lexical = [[(doc(r), float(lex - i)) for i, r in enumerate(rng.choice(n, lex, replace=False))] for _ in range(nq)]
    return fast, qual, lexical


def _pair(rng, n, cluster=40):
    """A CLUSTERED fast tier (a pool of 30 then holds many rows that are each other's nearest neighbours, so the smoothing has
    edges to walk) and a random quality tier."""
    from frankensearch_amd.synthetic import random_bert_weights
    centres = rng.standard_normal((n // cluster, 256)).astype(F32)
    fast = centres[rng.permutation(n) % (n // cluster)] + F32(0.45) * rng.standard_normal((n, 256)).astype(F32)
    fast_slab = fast.astype(np.float16).view(np.uint16)
    qual_slab = rng.standard_normal((n, 384)).astype(np.float16).view(np.uint16)
    table = rng.standard_normal((5000, 256)).astype(F32)
    return fast_slab, qual_slab, table, random_bert_weights(5, 3000, 384, 2, 512)


def sbits(hits):
    return [None if h.semantic_score is None else int(bits(h.semantic_score).reshape(-1)[0]) for h in hits]


def same_list(got, want, what):
    assert [(h.doc_id, h.rrf_score) for h in got] == [(h.doc_id, h.rrf_score) for h in want], what
    assert sbits(got) == sbits(want), what
    if "initial" in what[0]:
        assert [h.semantic_index for h in got] == [h.semantic_index for h in want], what


class Pipeline:
    """tier answers -> hubness_ref's penalty WITHOUT a sort (if a table is given) -> smooth_ref, sorted once -> the library's RRF,
    blend and RRF, on given vectors"""

    def __init__(self, fa, fast, qual, lex, k, graph, alpha, m, mutual=False, r_d=None, beta=0.5):
        self.fa, self.fast, self.qual, self.lex, self.k, self.fetch = fa, fast, qual, lex, k, 3 * k
        self.graph, self.alpha, self.m, self.mutual, self.r_d, self.beta = graph, alpha, m, mutual, r_d, beta

    def __call__(self, qi, fvec, qvec, rescored):
        from frankensearch_amd import fusion
        r_, s_, c_ = self.fast.search_batch(fvec, self.fetch)
        raw = [(doc(r_[0, i]), float(s_[0, i]), int(r_[0, i])) for i in range(int(c_[0]))]
        pool = raw
        if self.r_d is not None:
            pool = H.apply_hubness_penalty(raw, self.r_d, self.beta, resort=False)
        fh = [(d, float(sc), i) for d, sc, i in R.neighbor_smooth(pool, self.graph, self.alpha, self.m, self.mutual, resort=True)]
        want_i = fusion.rrf_fuse(self.lex[qi], fh, self.k)
        if rescored:   # quality_scores_for_hits of the CORRECTED pool, position by position
            scores = self.qual.gather_dot(qvec, [i for _, _, i in fh])
            blended = fusion.blend_two_tier_aligned(fh, [float(x) for x in scores], 0.7)
        else:
            r_, s_, c_ = self.qual.search_batch(qvec, self.fetch)
            qh = [(doc(r_[0, i]), float(s_[0, i]), int(r_[0, i])) for i in range(int(c_[0]))]
            blended = fusion.blend_two_tier(fh, qh, 0.7)
            fidx = {d: i for d, _, i in fh}
            blended = [(d, sc, fidx.get(d, 0xFFFFFFFF)) for d, sc, _ in blended]
        return raw, fh, want_i, fusion.rrf_fuse(self.lex[qi], blended, self.k)


@pytest.fixture(scope="module")
def world():
    fa = _fa()
    rng = np.random.default_rng(1313)
    n, nq, k = 20_000, 96, 10
    fast_slab, qual_slab, table, w = _pair(rng, n)
    fast, qual = fa.VectorIndex.from_slab(fast_slab), fa.VectorIndex.from_slab(qual_slab)
    m2v, bert = fa.Model2VecEmbedder(table), fa.NativeEmbedder(w)
    fq, qq, lex = _queries(rng, nq, n)
    graph = fast.build_knn_graph(16)        # width 16: m = 10 walks a prefix, mutual mode scans all 16 columns
    sample = np.stack([m2v.embed_token_ids(t) for t in _queries(rng, 128, n)[0]])
    r_d = (fast.compute_query_hubness(sample, 10) * F32(0.25)).astype(F32)
    yield dict(fa=fa, n=n, nq=nq, k=k, fast=fast, qual=qual, m2v=m2v, bert=bert, fq=fq, qq=qq, lex=lex, graph=graph, r_d=r_d,
               fast_slab=fast_slab, qual_slab=qual_slab)
    for h in (fast, qual, m2v, bert):
        h.close()


@pytest.mark.parametrize("with_hubness", [False, True])
def test_searcher_with_a_graph_equals_the_host_side_pipeline(world, with_hubness):
    from frankensearch_amd.host import NativeTwoTierSearcher
    w = world
    fa, fast, qual, m2v, bert, fq, qq, lex, k, nq, graph = (w[x] for x in ("fa", "fast", "qual", "m2v", "bert", "fq", "qq", "lex", "k", "nq", "graph"))
    r_d = w["r_d"] if with_hubness else None
    never = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    if with_hubness:
        never.set_hubness(r_d, 0.5)
    base = never.search_many(fq, qq, k, lex, chunk=32)
    base_one = [never.search(fq[qi], qq[qi], k, lex[qi])[:2] for qi in range(0, nq, 12)]
    s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    resc = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, quality_pool=1)
    if with_hubness:
        s.set_hubness(r_d, 0.5)
        resc.set_hubness(r_d, 0.5)
    # an identity configuration, a detached or empty graph: byte-identical to a searcher that never had the call made (with a hubness
    # table attached: to the hubness-only searcher)
    for g, alpha, m in ((graph, 0.0, 10), (None, 0.3, 10), (graph[:0], 0.3, 10), (graph, float("nan"), 10), (graph, 0.3, 0), (graph, -1.0, 10)):
        s.set_neighbor_smoothing(g, alpha, m)
        got = s.search_many(fq, qq, k, lex, chunk=32)
        assert got[0] == base[0] and got[1] == base[1], (alpha, m)
        assert [s.search(fq[qi], qq[qi], k, lex[qi])[:2] for qi in range(0, nq, 12)] == base_one
    pipe = Pipeline(fa, fast, qual, lex, k, graph, 0.3, 10, r_d=r_d)
    s.set_neighbor_smoothing(graph, 0.3, 10)
    resc.set_neighbor_smoothing(graph, 0.3, 10)
    ini, fin, rf, st, fv, qv = s.search_many(fq, qq, k, lex, chunk=32, want_vectors=True)
    got_r = resc.search_many(fq, qq, k, lex, chunk=32, want_vectors=True)
    assert not rf.any() and not got_r[2].any()
    moved = rescored_scores = 0
    for qi in range(nq):
        raw, fh, want_i, want_f = pipe(qi, fv[qi], qv[qi], False)
        moved += [d for d, _, _ in fh] != [d for d, _, _ in raw]
        rescored_scores += sum(1 for a, b in zip(sorted(fh), sorted(raw)) if a[1] != b[1])
        same_list(ini[qi], want_i, ("many initial", qi))
        same_list(fin[qi], want_f, ("many final", qi))
        _, _, want_i, want_f = pipe(qi, got_r[4][qi], got_r[5][qi], True)
        same_list(got_r[0][qi], want_i, ("many rescored initial", qi))
        same_list(got_r[1][qi], want_f, ("many rescored final", qi))
    print(f"hubness {with_hubness}: pools the correction reordered {moved} of {nq}; scores it changed {rescored_scores}")
    assert moved >= nq // 2
    assert ini != base[0]
    # fshost_two_tier_search, query by query, on that call's own vectors
    one = {}
    for qi in range(0, nq, 6):
        fvec, qvec = m2v.embed_token_ids(fq[qi]), bert.embed_token_ids(qq[qi])
        i1, f1, _ = s.search(fq[qi], qq[qi], k, lex[qi])
        _, _, want_i, want_f = pipe(qi, fvec, qvec, False)
        same_list(i1, want_i, ("search initial", qi))
        same_list(f1, want_f, ("search final", qi))
        assert i1 == ini[qi], qi
        i2, f2, _ = resc.search(fq[qi], qq[qi], k, lex[qi])
        _, _, want_i, want_f = pipe(qi, fvec, qvec, True)
        same_list(i2, want_i, ("search rescored initial", qi))
        same_list(f2, want_f, ("search rescored final", qi))
        one[qi] = (i1, f1)
    # detaching restores the pre-attach results bit for bit
    s.set_neighbor_smoothing(None)
    got = s.search_many(fq, qq, k, lex, chunk=32)
    assert got[0] == base[0] and got[1] == base[1]
    assert [s.search(fq[qi], qq[qi], k, lex[qi])[:2] for qi in range(0, nq, 12)] == base_one
    if not with_hubness:
        # over sharded tiers: the sharded graph is the same table, the sharded searcher gives the same lists
        P = fa.NativeShardedIndex.EXCHANGE_PEER_COPY
        sfast = fa.NativeShardedIndex.from_slab(w["fast_slab"], [0] * 2, exchange=P)
        squal = fa.NativeShardedIndex.from_slab(w["qual_slab"], [0] * 2, exchange=P)
        assert np.array_equal(sfast.build_knn_graph(16, first_row=9_000, n_rows=2_000), graph[9_000:11_000])
        sh = NativeTwoTierSearcher(sfast, squal, m2v, bert, doc_id_mode=1)
        sh.set_neighbor_smoothing(graph, 0.3, 10)
        got = sh.search_many(fq, qq, k, lex, chunk=32)
        assert got[0] == ini and got[1] == fin
        for qi in range(0, nq, 24):
            assert tuple(sh.search(fq[qi], qq[qi], k, lex[qi])[:2]) == one[qi], qi
        for h in (sh, sfast, squal):
            h.close()
    for h in (never, s, resc):
        h.close()


def test_mutual_mode(world):
    from frankensearch_amd.host import NativeTwoTierSearcher
    w = world
    fa, fast, qual, m2v, bert, fq, qq, lex, k, nq, graph = (w[x] for x in ("fa", "fast", "qual", "m2v", "bert", "fq", "qq", "lex", "k", "nq", "graph"))
    s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1)
    s.set_neighbor_smoothing(graph, 0.3, 10, mutual=False)
    plain = s.search_many(fq, qq, k, lex, chunk=32)[:2]
    s.set_neighbor_smoothing(graph, 0.3, 10, mutual=True)
    ini, fin, rf, st, fv, qv = s.search_many(fq, qq, k, lex, chunk=32, want_vectors=True)
    pipe = Pipeline(fa, fast, qual, lex, k, graph, 0.3, 10, mutual=True)
    for qi in range(nq):
        _, _, want_i, want_f = pipe(qi, fv[qi], qv[qi], False)
        same_list(ini[qi], want_i, ("mutual initial", qi))
        same_list(fin[qi], want_f, ("mutual final", qi))
    differing = sum(a != b for a, b in zip(ini, plain[0]))
    print(f"queries whose initial list differs between mutual and plain smoothing: {differing} of {nq}")
    assert differing > 0
    s.close()


def test_a_graph_swapped_during_searches_never_splits_a_search(world):
    """A thread swaps two graphs (and two alphas) as fast as it can while search_many runs in RescoredFastPool mode, where the
    quality scores are stored by position in the corrected pool.  Every call equals, whole, the answer under one snapshot or the
    other; per-query callers riding the batching engine get an initial list that is one of the two."""
    from frankensearch_amd.host import NativeTwoTierSearcher
    w = world
    fast, qual, m2v, bert, fq, qq, lex, k, nq, graph = (w[x] for x in ("fast", "qual", "m2v", "bert", "fq", "qq", "lex", "k", "nq", "graph"))
    other = np.ascontiguousarray(graph[:, :3])
    s = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=1, quality_pool=1)
    s.set_neighbor_smoothing(graph, 0.3, 10)
    under_a = s.search_many(fq, qq, k, lex, chunk=16)[:2]
    s.set_neighbor_smoothing(other, 0.6, 10)
    under_b = s.search_many(fq, qq, k, lex, chunk=16)[:2]
    assert under_a[0] != under_b[0] and under_a[1] != under_b[1]
    stop, swaps = threading.Event(), [0]

    def toggle():
        while not stop.is_set():
            if swaps[0] % 2:
                s.set_neighbor_smoothing(other, 0.6, 10)
            else:
                s.set_neighbor_smoothing(graph, 0.3, 10)
            swaps[0] += 1

    t = threading.Thread(target=toggle)
    t.start()
    try:
        seen = {"a": 0, "b": 0}
        for _ in range(10):
            got = s.search_many(fq, qq, k, lex, chunk=16)[:2]
            which = "a" if got[0] == under_a[0] else "b"
            assert (got[0], got[1]) == ((under_a[0], under_a[1]) if which == "a" else (under_b[0], under_b[1]))
            seen[which] += 1
        s.set_batching(32, 500)
        bad = []

        def caller(lo):
            for qi in range(lo, nq, 8):
                i1, _, _ = s.search(fq[qi], qq[qi], k, lex[qi])
                if i1 != under_a[0][qi] and i1 != under_b[0][qi]:
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
    print(f"{swaps[0]} swaps during 10 calls; calls answered under graph A {seen['a']}, under graph B {seen['b']}")
    assert swaps[0] > 20
    s.close()


def test_a_resident_wal_entry_in_the_pool_is_unchanged(tmp_path):
    """The graph is over the main slab: a WAL hit's index lies past the table, so it has no edges and is nobody's neighbour."""
    fa = _fa()
    from frankensearch_amd import fusion
    from frankensearch_amd.host import NativeTwoTierSearcher
    from frankensearch_amd.synthetic import random_bert_weights
    rng = np.random.default_rng(77)
    n, k = 3_000, 10
    centres = rng.standard_normal((n // 30, 256)).astype(F32)
    fvecs = centres[rng.permutation(n) % (n // 30)] + F32(0.45) * rng.standard_normal((n, 256)).astype(F32)
    ids = [f"doc-{i:05d}" for i in range(n)]
    pf, pq = str(tmp_path / "fast.fsvi"), str(tmp_path / "qual.fsvi")
    fa.write_fsvi(pf, list(zip(ids, fvecs)), "potion", "r1")
    fa.write_fsvi(pq, list(zip(ids, rng.standard_normal((n, 384)).astype(F32))), "minilm", "r1")
    fast, qual = fa.VectorIndex.open(pf), fa.VectorIndex.open(pq)
    m2v = fa.Model2VecEmbedder(rng.standard_normal((5000, 256)).astype(F32))
    bert = fa.NativeEmbedder(random_bert_weights(5, 3000, 384, 2, 512))
    fast_ids, quality_ids = rng.integers(0, 5000, 9).tolist(), [101, 1500, 1600, 102]
    fvec = m2v.embed_token_ids(fast_ids)
    fast.append("fresh", fvec * F32(30.0 / np.linalg.norm(fvec)))   # a resident WAL entry that points straight at the query, longer than any row
    assert fast.wal_record_count() == 1
    graph = fast.build_knn_graph(10)
    assert graph.shape == (n, 10)                           # the main rows only
    s = NativeTwoTierSearcher(fast, qual, m2v, bert)        # doc-id tables: search_hits merges the WAL entry into the pool
    before = s.search(fast_ids, quality_ids, k, [])[0]
    s.set_neighbor_smoothing(graph, 0.3, 10)
    after = s.search(fast_ids, quality_ids, k, [])[0]
    pool = fast.search_top_k(fvec, 3 * k)
    raw = [(h.doc_id, h.score, h.index) for h in pool]
    wal = [h for h in raw if h[0] == "fresh"]
    assert len(wal) == 1 and wal[0][2] >= n                 # a virtual row past the table
    want = R.neighbor_smooth(raw, graph, 0.3, 10, resort=True)
    same_list(after, fusion.rrf_fuse([], [(d, float(sc), i) for d, sc, i in want], k), ("initial with a WAL hit", 0))
    b = {h.doc_id: h.semantic_score for h in before}
    a = {h.doc_id: h.semantic_score for h in after}
    b1 = lambda x: int(bits(x).reshape(-1)[0])
    assert "fresh" in a and b1(a["fresh"]) == b1(b["fresh"]) == b1(wal[0][1])
    assert any(d in b and b1(a[d]) != b1(b[d]) for d in a if d != "fresh"), "the smoothing changed no main hit"
    for h in (s, fast, qual, m2v, bert):
        h.close()

"""GPU checks of MMR over index rows (mmr_kernels.hip): the device path against tests/mmr_ref.py and against fsgpu_mmr_rerank fed with
fsgpu_index_vector_at_f32 of the same rows — identical order, similarity matrix equal bit for bit, no tolerance —, batch invariance,
the pool sizes at and past the device limits, the docs / two-tier forms and the searcher's stage."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import mmr_ref as M  # noqa: E402

pytestmark = pytest.mark.gpu


def _fa():
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))))


def _f16_index(rng, n, dim):
    fa = _fa()
    vec = M.clustered(rng, n, dim, centroids=40, dtype="f16")
    return fa.VectorIndex.from_slab(vec.astype(np.float16)), vec


def _f32_index(rng, n, dim, tmp_path, name="f32.fsvi"):
    """An F32-quantised FSVI file: rows come back sorted by doc-id hash, so the vectors are read back by doc id."""
    fa = _fa()
    vec = M.clustered(rng, n, dim, centroids=40, dtype="f32")
    ids = [f"doc-{i:05d}" for i in range(n)]
    path = str(tmp_path / name)
    fa.write_fsvi(path, list(zip(ids, vec)), quantization=0)
    idx = fa.VectorIndex.open(path)
    by_id = dict(zip(ids, vec))
    rows = np.stack([by_id[idx.doc_id_at(r)] for r in range(n)])
    return idx, rows


def _check_pool(idx, vec, rows, scores, k, cfg):
    """device order + sims == restatement == fsgpu_mmr_rerank on vector_at of the same rows"""
    fa = _fa()
    got, sims = idx.mmr_rerank(rows, scores, k, cfg, want_sims=True)
    want, want_sims = M.mmr_rerank(list(scores), list(vec[rows]), k, cfg.lambda_, cfg.candidate_pool)
    fetched = [idx.vector_at(int(r)) for r in rows[:min(len(rows), cfg.candidate_pool)]]
    host, host_sims = fa.mmr_rerank(scores[:len(fetched)], fetched, k, cfg, want_sims=True)
    print(f"pool {len(rows)} x {vec.shape[1]}: sims differing from the restatement "
          f"{int(np.sum(bits(sims) != bits(want_sims)))}, from the host path {int(np.sum(bits(sims) != bits(host_sims)))}")
    assert got.tolist() == want and host.tolist() == want
    assert same_bits(sims, want_sims) and same_bits(host_sims, want_sims)
    assert np.array_equal(idx.mmr_rerank(rows, scores, k, cfg), got)   # the LDS-matrix launch: same order
    return got


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_device_equals_restatement_and_host_path_bit_for_bit(quant, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(11)
    n, dim = 3000, 384
    idx, vec = _f16_index(rng, n, dim) if quant == "f16" else _f32_index(rng, n, dim, tmp_path)
    for r in (0, 1, n // 2, n - 1):
        assert np.array_equal(idx.vector_at(r).view(np.uint32), vec[r].view(np.uint32))   # vector_at_f32 == the widened slab
    with pytest.raises(fa.InvalidConfig):
        idx.vector_at(n)
    moved = 0
    for trial, size in enumerate((1, 2, 30, 30, 30, 64, 128)):
        # rows around a few anchors, as a top-k answer is: near-duplicates that MMR pushes down
        anchor = vec[rng.integers(0, n, 3)]
        near = np.argsort(-(vec @ anchor.T).max(axis=1))[:max(size * 2, 4)]
        rows = rng.permutation(near)[:size].astype(np.uint32)
        scores = M.scores_for(rng, size, ("plain", "ties", "nonfinite", "plain", "negative", "plain", "ties")[trial])
        cfg = fa.MmrConfig(True, (0.7, 0.5, 0.3, 0.7, 0.6, 0.5, 0.7)[trial], 1000)
        got = _check_pool(idx, vec, rows, scores, size, cfg)
        moved += size >= 30 and got.tolist() != list(range(size))
    assert moved >= 3
    # k below the pool, the candidate pool below the list, k = 0, an empty list, a row out of range
    rows = rng.choice(n, 40, replace=False).astype(np.uint32)
    scores = M.scores_for(rng, 40, "plain")
    _check_pool(idx, vec, rows, scores, 10, fa.MmrConfig(True, 0.7, 30))
    assert idx.mmr_rerank(rows, scores, 0, fa.MmrConfig(True)).size == 0
    assert idx.mmr_rerank([], [], 5, fa.MmrConfig(True)).size == 0
    with pytest.raises(fa.InvalidConfig):
        idx.mmr_rerank([n], [1.0], 1, fa.MmrConfig(True))


def test_pool_past_the_device_limit_runs_the_host_restatement_with_the_same_bits(tmp_path):
    fa = _fa()
    rng = np.random.default_rng(12)
    idx, vec = _f16_index(rng, 600, 384)
    for size in (128, 129, 200):   # 128 x 384 is the device's largest; 129 and 200 fall back
        rows = rng.choice(600, size, replace=False).astype(np.uint32)
        _check_pool(idx, vec, rows, M.scores_for(rng, size, "plain"), size, fa.MmrConfig(True, 0.7, 1000))
    # 64 x 1,024 on the device (the staged rows leave no room for the matrix in LDS), 65 x 1,024 on the host; f32 rows of that
    # size are staged in the global workspace
    for quant in ("f16", "f32"):
        idx, vec = _f16_index(rng, 200, 1024) if quant == "f16" else _f32_index(rng, 200, 1024, tmp_path, "wide.fsvi")
        for size in (64, 65):
            rows = rng.choice(200, size, replace=False).astype(np.uint32)
            _check_pool(idx, vec, rows, M.scores_for(rng, size, "ties"), size, fa.MmrConfig(True, 0.5, 1000))
    # a batch that mixes device pools and a host pool
    idx, vec = _f16_index(rng, 600, 384)
    sizes = [30, 150, 2, 128]
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    rows = rng.integers(0, 600, int(offs[-1])).astype(np.uint32)
    scores = rng.random(int(offs[-1]))
    cfg = fa.MmrConfig(True, 0.6, 1000)
    got = idx.mmr_rerank_batched(rows, scores, offs, 1000, cfg)
    for q, size in enumerate(sizes):
        sl = slice(int(offs[q]), int(offs[q + 1]))
        assert got[q].tolist() == M.mmr_rerank(list(scores[sl]), list(vec[rows[sl]]), 1000, 0.6, 1000)[0], q


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_dimension_15(quant, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(13)
    idx, vec = _f16_index(rng, 500, 15) if quant == "f16" else _f32_index(rng, 500, 15, tmp_path)
    for size in (2, 30, 128):
        rows = rng.choice(500, size, replace=False).astype(np.uint32)
        _check_pool(idx, vec, rows, M.scores_for(rng, size, "plain"), size, fa.MmrConfig(True, 0.5, 1000))


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_batch_invariance(quant, tmp_path):
    """A pool alone, inside 1,024 pools, in reversed batch order, split over two calls: identical orders."""
    fa = _fa()
    rng = np.random.default_rng(14)
    n, dim, nq = 20000, 384, 1024
    idx, vec = _f16_index(rng, n, dim) if quant == "f16" else _f32_index(rng, 4000, dim, tmp_path)
    n = vec.shape[0]
    sizes = rng.integers(1, 41, nq)
    sizes[:4] = (30, 1, 128, 2)
    offs = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint32)
    rows = np.concatenate([(int(rng.integers(0, n - 300)) + rng.permutation(300)[:s]) for s in sizes]).astype(np.uint32)
    scores = np.concatenate([M.scores_for(rng, int(s), "ties" if i % 3 == 0 else "plain") for i, s in enumerate(sizes)])
    cfg = fa.MmrConfig(True, 0.7, 30)
    k = 30
    whole = idx.mmr_rerank_batched(rows, scores, offs, k, cfg)
    assert len(whole) == nq and all(len(o) == min(k, s) for o, s in zip(whole, sizes))
    for q in (0, 1, 2, 3, 17, 500, nq - 1):   # alone, and against the restatement
        sl = slice(int(offs[q]), int(offs[q + 1]))
        alone = idx.mmr_rerank(rows[sl], scores[sl], k, cfg)
        assert alone.tolist() == whole[q].tolist(), q
        assert alone.tolist() == M.mmr_rerank(list(scores[sl]), list(vec[rows[sl]]), k, 0.7, 30)[0], q
    # reversed batch order
    rev_sizes = sizes[::-1]
    rev_offs = np.concatenate([[0], np.cumsum(rev_sizes)]).astype(np.uint32)
    rev_rows = np.concatenate([rows[int(offs[q]):int(offs[q + 1])] for q in range(nq - 1, -1, -1)])
    rev_scores = np.concatenate([scores[int(offs[q]):int(offs[q + 1])] for q in range(nq - 1, -1, -1)])
    rev = idx.mmr_rerank_batched(rev_rows, rev_scores, rev_offs, k, cfg)
    assert all(rev[nq - 1 - q].tolist() == whole[q].tolist() for q in range(nq))
    # split over two calls
    cut = 411
    a = idx.mmr_rerank_batched(rows[:int(offs[cut])], scores[:int(offs[cut])], offs[:cut + 1], k, cfg)
    b = idx.mmr_rerank_batched(rows[int(offs[cut]):], scores[int(offs[cut]):], offs[cut:] - offs[cut], k, cfg)
    assert all(x.tolist() == y.tolist() for x, y in zip(a + b, whole))
    assert sum(o.tolist() != list(range(len(o))) for o in whole) >= nq // 3   # MMR moved a good share of the pools


def _doc_index(rng, tmp_path, name, n=400, dim=128, quantization=1):
    fa = _fa()
    vec = M.clustered(rng, n, dim, centroids=12, dtype="f16" if quantization == 1 else "f32")
    ids = [f"doc-{i:04d}" for i in range(n)]
    path = str(tmp_path / name)
    fa.write_fsvi(path, list(zip(ids, vec)), quantization=quantization)
    return fa.VectorIndex.open(path), ids, dict(zip(ids, vec))


@pytest.mark.parametrize("quantization", [1, 0])
def test_docs_form_wal_shadow_tombstone_and_missing_document(quantization, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(15)
    idx, ids, by_id = _doc_index(rng, tmp_path, "docs.fsvi", quantization=quantization)
    cfg = fa.MmrConfig(True, 0.6, 30)
    pick = [ids[i] for i in rng.choice(len(ids), 40, replace=False)]
    docs = [(d, float(np.float32(1.0 - 0.02 * i))) for i, d in enumerate(pick)]

    def expect(vectors):
        order, _ = M.mmr_rerank([float(np.float32(s)) for _, s in docs[:30]], [vectors[d] for d, _ in docs[:30]], 30, 0.6, 30)
        return order + list(range(30, 40))
    order, applied = idx.mmr_rerank_docs(docs, cfg)
    assert applied and order == expect(by_id) and order != list(range(40))
    # a WAL entry shadows its main row: the newest entry's f32 vector is what MMR reads
    shadow = dict(by_id)
    wal_vec = M.clustered(rng, 1, 128, dtype="f32")[0]
    idx.append(pick[3], M.clustered(rng, 1, 128, dtype="f32")[0])
    idx.append(pick[3], wal_vec)
    shadow[pick[3]] = wal_vec
    fresh = M.clustered(rng, 1, 128, dtype="f32")[0]
    idx.append("doc-new", fresh)       # a document that exists only in the WAL
    shadow["doc-new"] = fresh
    docs[7] = ("doc-new", docs[7][1])
    order, applied = idx.mmr_rerank_docs(docs, cfg)
    assert applied and order == expect(shadow)
    # a tombstoned document resolves to nothing: the pool is incomplete, the list stays as it is
    assert idx.soft_delete(pick[5])
    order, applied = idx.mmr_rerank_docs(docs, cfg)
    assert not applied and order == list(range(40))
    docs[5] = (pick[35], docs[5][1])   # ... past the pool it does not matter
    docs[35] = (pick[5], docs[35][1])
    order, applied = idx.mmr_rerank_docs(docs, cfg)
    assert applied and order == expect(shadow)
    docs[2] = ("no-such-doc", docs[2][1])
    order, applied = idx.mmr_rerank_docs(docs, cfg)
    assert not applied and order == list(range(40))
    # disabled, one result, a pool of one
    assert idx.mmr_rerank_docs(docs, fa.MmrConfig(False, 0.6, 30)) == (list(range(40)), False)
    assert idx.mmr_rerank_docs(docs[:1], cfg) == ([0], False)
    assert idx.mmr_rerank_docs(docs, fa.MmrConfig(True, 0.6, 0)) == (list(range(40)), False)


def test_two_tier_all_quality_all_fast_and_mixed(tmp_path):
    fa = _fa()
    from frankensearch_amd.two_tier import TwoTierIndex
    rng = np.random.default_rng(16)
    n = 300
    ids = [f"doc-{i:04d}" for i in range(n)]
    fast_vec = M.clustered(rng, n, 64, centroids=10, dtype="f16")
    qual_vec = M.clustered(rng, n, 128, centroids=10, dtype="f16")
    have_quality = set(ids[:200])   # the last 100 documents have no quality vector
    pf, pq = str(tmp_path / "fast.fsvi"), str(tmp_path / "qual.fsvi")
    fa.write_fsvi(pf, list(zip(ids, fast_vec)))
    fa.write_fsvi(pq, [(d, v) for d, v in zip(ids, qual_vec) if d in have_quality])
    fast, qual = fa.VectorIndex.open(pf), fa.VectorIndex.open(pq)
    pair = TwoTierIndex(fast, qual)
    fv, qv = dict(zip(ids, fast_vec)), dict(zip(ids, qual_vec))
    cfg = fa.MmrConfig(True, 0.6, 30)

    def run(pick):
        hits = [(d, float(np.float32(1.0 - 0.03 * i))) for i, d in enumerate(pick)]
        vectors = [qv[d] if d in have_quality else fv[d] for d in pick[:30]]
        want, _ = M.mmr_rerank([float(np.float32(s)) for _, s in hits[:30]], vectors, 30, 0.6, 30)
        order, applied = pair.mmr_rerank(hits, cfg)
        assert applied and order == want + list(range(30, len(pick)))
        return order
    all_q = run([ids[i] for i in rng.choice(200, 36, replace=False)])
    all_f = run([ids[200 + i] for i in rng.choice(100, 36, replace=False)])
    mixed = run([ids[i] for i in rng.permutation(np.concatenate([rng.choice(200, 20, replace=False), 200 + rng.choice(100, 16, replace=False)]))])
    assert sum(o != list(range(36)) for o in (all_q, all_f, mixed)) >= 2
    # mmr_step over the pair: head reordered, tail in place; a document in neither tier leaves the list as it is
    pick = [ids[i] for i in rng.choice(200, 36, replace=False)]
    items = [(d, 1.0 - 0.03 * i, "payload") for i, d in enumerate(pick)]
    out, applied = fa.mmr_step(items, pair, cfg)
    assert applied and [o[0] for o in out[30:]] == pick[30:] and sorted(o[0] for o in out) == sorted(pick)
    out, applied = fa.mmr_step([("ghost", 2.0, "x")] + items, pair, cfg)
    assert not applied and out == [("ghost", 2.0, "x")] + items


def test_mmr_step_after_rerank_step_end_to_end(tmp_path):
    """searcher.rs: rerank_step_with_combine, then the MMR stage on its output."""
    fa = _fa()
    import reranker_ref as R
    from oracle import bert_oracle
    from frankensearch_amd.rerank import PURE_REORDER, RerankCandidate, rerank_step
    rng = np.random.default_rng(17)
    w = bert_oracle.random_weights(5, 500, 128, 2, 512)
    w.update(R.head_weights(9, 128))
    model = fa.NativeReranker(w)
    idx, ids, by_id = _doc_index(rng, tmp_path, "e2e.fsvi")
    pick = [ids[i] for i in rng.choice(len(ids), 24, replace=False)]
    pairs = {d: R.make_pair(rng, 500, 5, int(rng.integers(1, 40))) for d in pick}
    cands = [RerankCandidate(d, 1.0 - 0.03 * i, None, i) for i, d in enumerate(pick)]
    ranked, applied, err = rerank_step(model, cands, pairs.get, top_k_rerank=20, min_candidates=5, combine=PURE_REORDER)
    assert applied and err is None
    cfg = fa.MmrConfig(True, 0.5, 16)
    out, applied = fa.mmr_step(ranked, idx, cfg)
    assert applied
    want, _ = M.mmr_rerank([float(np.float32(c.score)) for c in ranked[:16]], [by_id[c.doc_id] for c in ranked[:16]], 16, 0.5, 16)
    assert [c.doc_id for c in out] == [ranked[i].doc_id for i in want] + [c.doc_id for c in ranked[16:]]
    assert fa.mmr_step(ranked, idx, fa.MmrConfig(False, 0.5, 16)) == (ranked, False)


def test_searcher_unchanged_without_mmr_and_diversified_with_it():
    fa = _fa()
    from oracle import bert_oracle
    from frankensearch_amd.two_tier import POOL_RESCORED, SyncTwoTierSearcher, TwoTierConfig
    rng = np.random.default_rng(18)
    n = 6000
    fast_vec = M.clustered(rng, n, 256, centroids=30, noise=0.2, dtype="f16")
    qual_vec = M.clustered(rng, n, 128, centroids=30, noise=0.2, dtype="f16")
    table = rng.standard_normal((2000, 256)).astype(np.float32)
    w = bert_oracle.random_weights(5, 3000, 128, 2, 512)
    doc = lambda r: f"doc-{r:08d}"
    s = SyncTwoTierSearcher(fa.VectorIndex.from_slab(fast_vec.astype(np.float16)), fa.VectorIndex.from_slab(qual_vec.astype(np.float16)),
                            fa.Model2VecEmbedder(table), fa.NativeEmbedder(w), doc, TwoTierConfig(quality_pool=POOL_RESCORED))
    changed = 0
    for trial in range(4):
        fast_ids = rng.integers(0, 2000, 9).tolist()
        qual_ids = [101] + rng.integers(1000, 3000, 10).tolist() + [102]
        base = s.search(fast_ids, qual_ids, 10, [])
        assert s.search(fast_ids, qual_ids, 10, [], mmr=None).final_results == base.final_results
        assert s.search(fast_ids, qual_ids, 10, [], mmr=fa.MmrConfig(False, 0.3, 30)).final_results == base.final_results
        div = s.search(fast_ids, qual_ids, 10, [], mmr=fa.MmrConfig(True, 0.3, 30))
        assert div.initial_results == base.initial_results
        assert sorted(h.doc_id for h in div.final_results) == sorted(h.doc_id for h in base.final_results)
        final = base.final_results
        want, _ = M.mmr_rerank([float(np.float32(h.rrf_score)) for h in final], [qual_vec[int(h.doc_id[4:])] for h in final], len(final), 0.3, 30)
        assert [h.doc_id for h in div.final_results] == [final[i].doc_id for i in want]
        changed += div.final_results != base.final_results
    assert changed >= 2

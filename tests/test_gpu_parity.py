"""GPU parity tests: libfsgpu.so (through the C ABI) vs the CPU oracle on the same inputs.

Bar: BIT-EXACT row ids and BIT-EXACT f32 score bits (the HIP scan reproduces the reference's
accumulation order), far inside the north-star's 1e-3 score tolerance.
Run on the GPU box with `pytest -m gpu`.
"""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    assert fa_mod._lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    return fa_mod


@pytest.fixture(params=["int8 filter", "f16 filter"])
def batched_filter(request, fa):
    """The batched search under each of its two filters (include/fsgpu.h, FSGPU_FILTER_*): every index a test creates is pinned
    to it; the results must be the exact search's either way."""
    fa.VectorIndex.default_batched_filter = 2 if request.param == "int8 filter" else 1
    yield request.param
    fa.VectorIndex.default_batched_filter = 0


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def rand_slab(rng, n, dim, scale=1.0):
    return (rng.standard_normal((n, dim)) * scale).astype(np.float16).view(np.uint16)


def assert_same(fa, oracle, slab, queries, k, live=None, allow=None, hreduce=0, variant=0):
    idx = fa.VectorIndex.from_slab(slab, live=live)
    idx.set_hreduce(hreduce)
    idx.set_variant(variant)
    rows, scores, counts = idx.search_batch(queries, k, allow=allow)
    eff_live = None
    if live is not None or allow is not None:
        eff_live = np.ones(slab.shape[0], bool)
        if live is not None:
            eff_live &= live
        if allow is not None:
            eff_live &= allow
    for qi in range(queries.shape[0]):
        er, es = oracle.search_top_k(slab, queries[qi], k, live=eff_live, hreduce=hreduce)
        n = int(counts[qi])
        assert n == len(er), (n, len(er))
        assert np.array_equal(rows[qi, :n], er), f"rows differ q={qi} k={k} shape={slab.shape}"
        assert np.array_equal(bits(scores[qi, :n]), bits(es)), f"score bits differ q={qi}"
    idx.close()


# ------------------------------------------------------------------------------------------------
def test_widen_f16_all_patterns_bit_exact(fa, oracle):
    # simd.rs:2711-2744
    src = np.arange(65536, dtype=np.uint16)
    got = fa.widen_f16_to_f32(src)
    ref = src.view(np.float16).astype(np.float32)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(np.signbit(got[nan]), np.signbit(ref[nan]))
    assert np.array_equal(got[~nan].view(np.uint32), ref[~nan].view(np.uint32))


def test_encode_f32_to_f16_matches_oracle(fa, oracle):
    # simd.rs:2245-2305 / :2669
    rng = np.random.default_rng(3)
    vals = np.concatenate([
        rng.standard_normal(100000).astype(np.float32),
        (rng.standard_normal(20000) * 1e-5).astype(np.float32),
        (rng.standard_normal(5000) * 7e4).astype(np.float32),
        np.array([0.0, -0.0, 1.0, 0.8, 0.2, 65504.0, 65520.0, 2.0 ** -24, 2.0 ** -25, 1.5 * 2.0 ** -25, np.inf,
                  -np.inf], dtype=np.float32),
        rng.integers(0, 2 ** 32, 100000, dtype=np.uint64).astype(np.uint32).view(np.float32),
    ])
    got = fa.encode_f32_to_f16(vals)
    want = oracle.encode_f32_to_f16(vals)
    nan = np.isnan(vals)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.all((got[nan] & 0x7C00) == 0x7C00) and np.all((got[nan] & 0x03FF) != 0)


@pytest.mark.parametrize("dim", [8, 16, 24, 40, 72, 128, 256, 384, 512, 768])
def test_scan_parity_dims(fa, oracle, dim):
    rng = np.random.default_rng(dim)
    for n in (1, 15, 16, 17, 1000, 4099):
        slab = rand_slab(rng, n, dim)
        q = rng.standard_normal((3, dim)).astype(np.float32)
        for k in (1, 10):
            assert_same(fa, oracle, slab, q, k)


@pytest.mark.parametrize("dim", [4, 7, 12, 100, 390])
def test_scan_parity_unaligned_dims_general_path(fa, oracle, dim):
    # dim % 8 != 0: scalar fused tail (simd.rs:441-445), rows not 16-byte aligned
    rng = np.random.default_rng(dim)
    for n in (3, 257, 3000):
        slab = rand_slab(rng, n, dim)
        q = rng.standard_normal((2, dim)).astype(np.float32)
        assert_same(fa, oracle, slab, q, 7)


@pytest.mark.parametrize("k", [1, 2, 10, 30, 60, 64, 65, 100, 256, 257, 300, 1000])
def test_scan_parity_k_tiers(fa, oracle, k):
    rng = np.random.default_rng(k)
    slab = rand_slab(rng, 20011, 128)
    q = rng.standard_normal((2, 128)).astype(np.float32)
    assert_same(fa, oracle, slab, q, k)


@pytest.mark.parametrize("nq", [1, 2, 3, 4, 5, 8, 9])
def test_scan_parity_query_batches(fa, oracle, nq):
    rng = np.random.default_rng(nq)
    for dim in (384, 256):
        slab = rand_slab(rng, 30000, dim)
        q = rng.standard_normal((nq, dim)).astype(np.float32)
        assert_same(fa, oracle, slab, q, 10)
        assert_same(fa, oracle, slab, q, 100)


def test_scan_parity_tombstones_and_allow_bitmap(fa, oracle):
    # search.rs:2163-2233 tombstones; filter.rs:19-56 as an allow bitmap
    rng = np.random.default_rng(17)
    slab = rand_slab(rng, 10007, 384)
    q = rng.standard_normal((4, 384)).astype(np.float32)
    live = rng.random(10007) > 0.3
    allow = rng.random(10007) > 0.5
    assert_same(fa, oracle, slab, q, 10, live=live)
    assert_same(fa, oracle, slab, q, 10, allow=allow)
    assert_same(fa, oracle, slab, q, 50, live=live, allow=allow)
    none_live = np.zeros(10007, bool)
    assert_same(fa, oracle, slab, q, 10, live=none_live)
    few = np.zeros(10007, bool)
    few[[5, 77, 9000]] = True
    assert_same(fa, oracle, slab, q, 10, live=few)
    assert_same(fa, oracle, slab, q, 400, live=live)  # general path with tombstones


def test_collect_all_and_k_above_n(fa, oracle):
    # search.rs:449-473 (k >= N), :2627-2643
    rng = np.random.default_rng(23)
    for n, dim in ((2, 8), (80, 8), (700, 128), (5000, 384)):
        slab = rand_slab(rng, n, dim)
        q = rng.standard_normal((2, dim)).astype(np.float32)
        assert_same(fa, oracle, slab, q, n)
        assert_same(fa, oracle, slab, q, n + 20)


def test_ties_nan_and_signed_zero_ordering(fa, oracle):
    # search.rs:2741-2764 ties by index; :2767-2787 NaN sorts last; total_cmp -0.0 < +0.0
    rng = np.random.default_rng(29)
    base = rand_slab(rng, 64, 128)
    slab = np.concatenate([base] * 40)  # every score appears 40 times -> pure index tie-breaks
    q = rng.standard_normal((2, 128)).astype(np.float32)
    for k in (1, 10, 64, 100, 300, slab.shape[0]):
        assert_same(fa, oracle, slab, q, k)
    qn = q.copy()
    qn[0, 3] = np.nan
    assert_same(fa, oracle, slab[:333], qn, 10)
    assert_same(fa, oracle, slab[:333], qn, 333)
    # rows of +inf / -inf / nan / zeros, and a query producing -0.0 and +0.0 scores
    special = np.zeros((48, 16), np.float16)
    special[1, 0] = np.inf
    special[2, 0] = -np.inf
    special[3, 0] = np.nan
    special[4, 0] = 1.0
    special[5, 0] = -1.0
    special[6, 0] = np.inf
    special[6, 1] = -np.inf
    slab2 = special.view(np.uint16)
    for qv in ([1.0] + [0.0] * 15, [-0.0] + [0.0] * 15, [0.0] * 16, [1.0, 1.0] + [0.0] * 14):
        q2 = np.array([qv], np.float32)
        for k in (5, 48):
            idx = fa.VectorIndex.from_slab(slab2)
            rows, scores, counts = idx.search_batch(q2, k)
            er, es = oracle.search_top_k(slab2, q2[0], k)
            n = int(counts[0])
            assert n == len(er) and np.array_equal(rows[0, :n], er)
            # NaN payload/sign is platform-defined (x86 default NaN is negative); compare NaN-ness + other bits
            gn, en = np.isnan(scores[0, :n]), np.isnan(es)
            assert np.array_equal(gn, en)
            assert np.array_equal(bits(scores[0, :n])[~gn], bits(es)[~en])


def test_hreduce_avx_order(fa, oracle):
    rng = np.random.default_rng(31)
    slab = rand_slab(rng, 5000, 384)
    q = rng.standard_normal((2, 384)).astype(np.float32)
    assert_same(fa, oracle, slab, q, 10, hreduce=1)
    assert_same(fa, oracle, slab, q, 300, hreduce=1)


def test_hreduce_sequential_order(fa, oracle):
    # FSGPU_HREDUCE_SEQ: f32x8::reduce_add as two left-to-right f32x4 sums (simd.rs:439,563; `wide` is not vendored)
    rng = np.random.default_rng(32)
    slab = rand_slab(rng, 5000, 384)
    q = rng.standard_normal((5, 384)).astype(np.float32)
    assert_same(fa, oracle, slab, q, 10, hreduce=2)
    assert_same(fa, oracle, slab, q, 300, hreduce=2)
    idx = fa.VectorIndex.from_slab(slab)
    idx.set_hreduce(2)
    many = rng.standard_normal((70, 384)).astype(np.float32)
    brows, bscores, _, _ = idx.search_batched(many, 10)
    for qi in (0, 13, 69):
        er, es = oracle.search_top_k(slab, many[qi], 10, hreduce=2)
        assert np.array_equal(brows[qi], er) and np.array_equal(bits(bscores[qi]), bits(es))


def test_runtime_dim_kernel_variant(fa, oracle):
    rng = np.random.default_rng(37)
    slab = rand_slab(rng, 9001, 384)
    q = rng.standard_normal((3, 384)).astype(np.float32)
    assert_same(fa, oracle, slab, q, 10, variant=1)


def test_reference_known_answers_through_fsvi(fa, oracle, tmp_path):
    # search.rs:2116-2137, 2163-2187, 2627-2643, 2741-2764 through the FSVI file + doc ids
    p = str(tmp_path / "kat.fsvi")
    assert oracle.fsvi_write(p, [("doc-a", [1.0, 0, 0, 0]), ("doc-b", [0.8, 0, 0, 0]), ("doc-c", [0.2, 0, 0, 0])]) == 0
    idx = fa.VectorIndex.open(p)
    assert idx.record_count() == 3 and idx.dimension() == 4
    hits = idx.search_top_k([1.0, 0, 0, 0], 2)
    assert [h.doc_id for h in hits] == ["doc-a", "doc-b"]
    assert [h.index for h in hits] == [0, 1]
    assert bits([h.score for h in hits]).tolist() == [0x3F800000, 0x3F4CC000]
    assert len(idx.search_top_k([1.0, 0, 0, 0], 20)) == 3
    assert idx.soft_delete("doc-a") and not idx.soft_delete("doc-a") and not idx.soft_delete("nope")
    hits = idx.search_top_k([1.0, 0, 0, 0], 10)
    assert [h.doc_id for h in hits] == ["doc-b", "doc-c"]
    with pytest.raises(fa.DimensionMismatch):
        idx.search_top_k([1.0, 0, 0], 2)
    # classified (search.rs:227-261)
    assert idx.search_top_k_classified([1.0, 0, 0, 0], 0).zero_signal == "CallerRequestedZeroK"
    assert idx.search_top_k_classified([0.0, 0, 0, 0], 3).zero_signal == "ZeroNormQuery"
    with pytest.raises(fa.InvalidConfig):
        idx.search_top_k_classified([np.inf, 0, 0, 0], 3)
    assert idx.search_top_k_classified([1.0, 0, 0, 0], 3).zero_signal is None
    # empty_result_reason (config.rs:696-740): all tombstoned -> WAL only -> (hit again)
    assert idx.soft_delete("doc-b") and idx.soft_delete("doc-c")
    assert idx.search_top_k_classified([1.0, 0, 0, 0], 3).zero_signal == "AllTombstoned"
    idx.append("w", [0.0, 1.0, 0, 0])
    got = idx.search_top_k_classified([1.0, 0, 0, 0], 3)
    assert got.zero_signal is None and [h.index for h in got.hits] == [3]
    assert idx.soft_delete("w")
    assert idx.search_top_k_classified([1.0, 0, 0, 0], 3).zero_signal == "AllTombstoned"
    pe = str(tmp_path / "empty.fsvi")
    fa.write_fsvi(pe, [])  # an empty writer.finish() (dimension 1)
    assert fa.VectorIndex.open(pe).search_top_k_classified([1.0], 3).zero_signal == "NewlyCreatedEmpty"
    idx = fa.VectorIndex.open(p)
    # NaN query through the unclassified path: all NaN, index ascending
    hits = idx.search_top_k([np.nan, 0, 0, 0], 3)
    assert all(np.isnan(h.score) for h in hits) and [h.index for h in hits] == sorted(h.index for h in hits)


def test_fsvi_file_parity_with_dedup_and_corruption(fa, oracle, tmp_path):
    rng = np.random.default_rng(41)
    rows = [(f"doc-{i % 180:03}", rng.standard_normal(64).astype(np.float32).tolist()) for i in range(200)]  # 20 dup ids
    p = str(tmp_path / "d.fsvi")
    assert oracle.fsvi_write(p, rows, "emb", "r1") == 0
    o = oracle.Fsvi(p)
    g = fa.VectorIndex.open(p)
    assert [g.doc_id_at(r) for r in range(200)] == [o.doc_id(r) for r in range(200)]
    for qi in range(5):
        q = rng.standard_normal(64).astype(np.float32)
        for k in (5, 40, 200):
            oh, os_ = o.search_top_k(q, k)
            gh = g.search_top_k(q, k)
            assert [(h.index, h.doc_id) for h in gh] == [(h[0], h[2]) for h in oh]
            assert np.array_equal(bits([h.score for h in gh]), bits(os_))
    raw = bytearray(open(p, "rb").read())
    for off, exc in ((20, fa.IndexCorrupted), (0, fa.IndexCorrupted), (4, fa.IndexVersionMismatch)):
        bad = bytearray(raw)
        bad[off] ^= 0x5A
        q = str(tmp_path / f"bad{off}.fsvi")
        open(q, "wb").write(bad)
        with pytest.raises(exc):
            fa.VectorIndex.open(q)
    with pytest.raises(fa.IoError):
        fa.VectorIndex.open(str(tmp_path / "missing.fsvi"))


def test_gather_dot_matches_oracle(fa, oracle):
    # lib.rs:3229-3239 / two_tier.rs:1566-1631
    rng = np.random.default_rng(43)
    for dim in (384, 40, 100, 7):
        slab = rand_slab(rng, 5000, dim)
        q = rng.standard_normal(dim).astype(np.float32)
        rows = rng.integers(0, 5000, 77).astype(np.uint32)
        idx = fa.VectorIndex.from_slab(slab)
        got = idx.gather_dot(q, rows)
        want = oracle.gather_dot(slab, q, rows)
        assert np.array_equal(bits(got), bits(want))
        assert bits([idx.dot_query_at(int(rows[0]), q)])[0] == bits(want[:1])[0]
        with pytest.raises(fa.InvalidConfig):
            idx.gather_dot(q, [5000])


def test_row_base_shards_merge_to_whole(fa, oracle):
    # contiguous row shards + global row ids => merged shard top-k == whole-index top-k
    rng = np.random.default_rng(47)
    n, dim, k = 30000, 384, 25
    slab = rand_slab(rng, n, dim)
    slab[100:110] = slab[20000:20010]  # cross-shard ties
    q = rng.standard_normal((3, dim)).astype(np.float32)
    whole = fa.VectorIndex.from_slab(slab)
    wr, ws, wc = whole.search_batch(q, k)
    cuts = [0, 7000, 15001, 15002, n]
    parts = [fa.VectorIndex.from_slab(slab[a:b], row_base=a) for a, b in zip(cuts[:-1], cuts[1:])]
    for qi in range(3):
        cand = []
        for p in parts:
            r, s, c = p.search_batch(q[qi:qi + 1], k)
            cand += [(int(r[0, i]), s[0, i]) for i in range(int(c[0]))]
        cand.sort(key=lambda t: (-(t[1] if not np.isnan(t[1]) else -np.inf), t[0]))
        assert [c[0] for c in cand[:k]] == wr[qi].tolist()
        assert np.array_equal(bits([c[1] for c in cand[:k]]), bits(ws[qi]))


def test_model2vec_bit_exact(fa, oracle):
    # model2vec_embedder.rs:691-849 formula model + random tables; :962-1010 invariants
    rng = np.random.default_rng(53)
    vocab, dim = 10, 8
    table = (np.arange(vocab, dtype=np.float32)[:, None] * np.float32(0.1)
             + np.arange(dim, dtype=np.float32)[None, :] * np.float32(0.01)).astype(np.float32)
    m = fa.Model2VecEmbedder(table)
    batch = [[1, 2, 3], [], [99, 100], [1, 99, 2], [0], [9, 9, 9, 9]]
    got = m.embed_batch_token_ids(batch)
    for i, ids in enumerate(batch):
        assert np.array_equal(bits(got[i]), bits(oracle.m2v_embed(table, ids))), i
    for vocab, dim in ((5000, 256), (3000, 128), (1000, 384)):
        table = rng.standard_normal((vocab, dim)).astype(np.float32)
        m = fa.Model2VecEmbedder(table)
        batch = [rng.integers(0, vocab + 50, int(rng.integers(0, 600))).tolist() for _ in range(40)]
        got = m.embed_batch_token_ids(batch)
        for i, ids in enumerate(batch):
            assert np.array_equal(bits(got[i]), bits(oracle.m2v_embed(table, ids))), (vocab, dim, i)


def test_config2_1m_x_384_clustered_corpus(fa, oracle):
    # BASELINE config 2: 1M x 384 f16, top-10, the reference's bench generator (fsvi_4bit_vs_incumbent.rs:56-101)
    n, dim = 1_000_000, 384
    slab = oracle.clustered_corpus_f16(0, n, dim)
    idx = fa.VectorIndex.from_slab(slab)
    queries = np.stack([oracle.clustered_query(q, dim) for q in range(6)])
    for k in (10, 30):
        rows, scores, counts = idx.search_batch(queries, k)
        for qi in range(queries.shape[0]):
            er, es = oracle.search_top_k(slab, queries[qi], k, nthreads=8)
            assert np.array_equal(rows[qi], er) and np.array_equal(bits(scores[qi]), bits(es))


def test_soft_delete_purges_resident_wal_entries(fa, oracle, tmp_path):
    # lib.rs:10064-10138 (soft_delete_removes_wal_only_record..., soft_delete_clears_pending_wal_updates_for_same_doc_id):
    # step 2 of soft_delete_batch (lib.rs:2358-2373) — same sequence on the oracle and on the GPU index
    p = str(tmp_path / "sd1.fsvi")
    oracle.fsvi_write(p, [("main-0", [1.0, 1.0, 1.0, 1.0])])
    g = fa.VectorIndex.open(p)
    g.append("wal-only", [0.0, 1.0, 0.0, 0.0])
    assert g.wal_record_count() == 1 and g.soft_delete("wal-only") and g.wal_record_count() == 0
    assert all(h.doc_id != "wal-only" for h in g.search_top_k([0.0, 1.0, 0.0, 0.0], 10))
    assert not g.soft_delete("wal-only")

    rng = np.random.default_rng(77)
    rows = [(f"doc-{i:03}", rng.standard_normal(16).astype(np.float32).tolist()) for i in range(120)]
    p2 = str(tmp_path / "sd2.fsvi")
    oracle.fsvi_write(p2, rows)
    o, g = oracle.Fsvi(p2), fa.VectorIndex.open(p2)
    for step in range(60):
        did = f"doc-{int(rng.integers(0, 140)):03}"
        if rng.random() < 0.5:
            v = rng.standard_normal(16).astype(np.float32)
            assert o.append(did, v) == 0
            g.append(did, v)
        else:
            assert o.soft_delete(did) == g.soft_delete(did), (step, did)
        assert o.wal_record_count == g.wal_record_count()
        q = rng.standard_normal(16).astype(np.float32)
        want, ws = o.search_top_k(q, 12)
        got = g.search_top_k(q, 12)
        assert [(h.index, h.doc_id) for h in got] == [(w[0], w[2]) for w in want], step
        assert np.array_equal(np.array([h.score for h in got], np.float32).view(np.uint32), ws.view(np.uint32))


def test_wal_overlay_matches_oracle(fa, oracle, tmp_path):
    # scan_wal + resolve (search.rs:1449-1475,1503-1596); repro_wal_shadow_bug.rs; search.rs:2688-2738
    p = str(tmp_path / "w.fsvi")
    oracle.fsvi_write(p, [("doc-a", [1.0, 0.0])])
    g = fa.VectorIndex.open(p)
    g.append("doc-a", [0.0, 1.0])
    hits = g.search_top_k([1.0, 0.0], 1)
    assert len(hits) == 1 and hits[0].doc_id == "doc-a" and abs(hits[0].score) < 1.2e-7 and hits[0].index == 1
    with pytest.raises(fa.DimensionMismatch):
        g.append("x", [1.0])
    with pytest.raises(fa.InvalidConfig):
        g.append("x", [np.nan, 0.0])
    with pytest.raises(fa.InvalidConfig):
        g.append("x", [0.0, 0.0])

    rng = np.random.default_rng(61)
    rows = [(f"doc-{i:03}", rng.standard_normal(40).astype(np.float32).tolist()) for i in range(300)]
    p2 = str(tmp_path / "w2.fsvi")
    oracle.fsvi_write(p2, rows)
    o = oracle.Fsvi(p2)
    g = fa.VectorIndex.open(p2)
    for j in range(25):
        did = f"doc-{(j * 7) % 300:03}" if j % 2 else f"new-{j}"
        v = rng.standard_normal(40).astype(np.float32)
        assert o.append(did, v) == 0
        g.append(did, v)
    assert g.wal_record_count() == o.wal_record_count
    for qi in range(6):
        q = rng.standard_normal(40).astype(np.float32)
        for k in (1, 5, 50, 400):
            oh, os_ = o.search_top_k(q, k)
            gh = g.search_top_k(q, k)
            assert [(h.index, h.doc_id) for h in gh] == [(h[0], h[2]) for h in oh]
            assert np.array_equal(bits([h.score for h in gh]), bits(os_))


def test_int8_two_pass_matches_oracle(fa, oracle, tmp_path):
    # search.rs:514-661; keep-all fixture (search.rs:1815-1859); slab quantiser simd.rs:1865-1886
    rng = np.random.default_rng(71)
    slab = oracle.encode_f32_to_f16(oracle.fixture_hashmix(300, 8))
    idx = fa.VectorIndex.from_slab(slab)
    for qi in range(8):
        q = np.array([(((qi * 7 + j * 3) % 11) / 11.0) - 0.5 for j in range(8)], dtype=np.float32)
        er, es = oracle.search_int8_two_pass(slab, q, 10, 50)
        gh = idx.search_top_k_int8_two_pass(q, 10, 50)
        assert [h.index for h in gh] == er.tolist() and np.array_equal(bits([h.score for h in gh]), bits(es))
    for n, dim in ((20000, 384), (7001, 256), (3000, 128), (5000, 40), (900, 768)):
        slab = rand_slab(rng, n, dim)
        si8 = oracle.quantize_slab_i8(slab)
        live = rng.random(n) > 0.1
        idx = fa.VectorIndex.from_slab(slab, live=live)
        for k, mult in ((10, 3), (1, 1), (30, 5), (64, 3), (100, 3), (10, 0)):
            q = rng.standard_normal(dim).astype(np.float32)
            er, es = oracle.search_int8_two_pass(slab, q, k, mult, live=live, slab_i8=si8)
            gh = idx.search_top_k_int8_two_pass(q, k, mult)
            assert [h.index for h in gh] == er.tolist(), (n, dim, k, mult)
            assert np.array_equal(bits([h.score for h in gh]), bits(es))
    # FSVI + WAL: falls back to the exact path (search.rs:579-585)
    p = str(tmp_path / "i8.fsvi")
    rows = [(f"doc-{i:03}", rng.standard_normal(64).astype(np.float32).tolist()) for i in range(200)]
    oracle.fsvi_write(p, rows)
    g, o = fa.VectorIndex.open(p), oracle.Fsvi(p)
    q = rng.standard_normal(64).astype(np.float32)
    er, es = oracle.search_int8_two_pass(o.slab(), q, 10, 3)
    gh = g.search_top_k_int8_two_pass(q, 10, 3)
    assert [h.index for h in gh] == er.tolist() and gh[0].doc_id == o.doc_id(int(er[0]))
    g.append("fresh", rng.standard_normal(64).astype(np.float32))
    o.append("fresh", np.zeros(64, np.float32) + 1)  # only to mirror the WAL presence
    assert [h.index for h in g.search_top_k_int8_two_pass(q, 10, 3)] == [h.index for h in g.search_top_k(q, 10)]


def test_batched_mfma_search_is_bit_exact(fa, oracle, batched_filter):
    # fsgpu_search_topk_batched must equal the exact path (hence the oracle) bit for bit
    rng = np.random.default_rng(83)
    for n, dim in ((200_000, 384), (150_001, 256), (60_000, 128)):
        cent = rng.standard_normal((32, dim)).astype(np.float32)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        rows = cent[rng.integers(0, 32, n)] + 0.3 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        slab = rows.astype(np.float16).view(np.uint16)
        live = rng.random(n) > 0.05
        idx = fa.VectorIndex.from_slab(slab, live=live)
        nq = 70
        q = cent[rng.integers(0, 32, nq)] + 0.3 * rng.standard_normal((nq, dim)).astype(np.float32) / np.sqrt(dim)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        q[5] = 0.0           # zero-norm query -> exact fallback
        q[6] *= 37.5         # non-unit query
        for k in (10, 1, 33):
            br, bs, bc, fb = idx.search_batched(q, k)
            er, es, ec = idx.search_batch(q, k)
            assert np.array_equal(bc, ec) and np.array_equal(br, er) and np.array_equal(bits(bs), bits(es)), (n, dim, k)
            assert fb < nq // 2, fb      # the matrix-core path must actually serve most queries
        # and against the oracle directly for a few
        for qi in (0, 6, 69):
            orow, osc = oracle.search_top_k(slab, q[qi], 10, live=live)
            br, bs, bc, _ = idx.search_batched(q, 10)
            assert np.array_equal(br[qi], orow) and np.array_equal(bits(bs[qi]), bits(osc))
    # small index / large k -> transparently the exact path
    slab = rand_slab(rng, 1500, 384)
    idx = fa.VectorIndex.from_slab(slab)
    q = rng.standard_normal((3, 384)).astype(np.float32)
    br, bs, bc, fb = idx.search_batched(q, 10)
    er, es, ec = idx.search_batch(q, 10)
    assert fb == 3 and np.array_equal(br, er) and np.array_equal(bits(bs), bits(es))


@pytest.mark.gpu
def test_batched_mfma_wide_groups_topical_rows_and_filters(fa, oracle, batched_filter):
    # 200 queries = one 128-query pass + one 64-query pass + a ragged tail; rows arrive in topical runs (sorted by
    # cluster), so a threshold sampled from the head of the slab would be useless — the strided samples must cope;
    # duplicates force score ties (lower row wins); an allow mask and k up to 64 ride along.
    rng = np.random.default_rng(97)
    n, dim = 300_037, 384
    cent = rng.standard_normal((48, dim)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    cid = np.sort(rng.integers(0, 48, n))
    rows = cent[cid] + 0.25 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[1000:1040] = rows[999]            # 41 identical rows
    rows[n - 5:] = rows[17]                # duplicates of an early row at the very end (partial last group)
    slab = rows.astype(np.float16).view(np.uint16)
    idx = fa.VectorIndex.from_slab(slab)
    nq = 200
    q = cent[rng.integers(0, 48, nq)] + 0.25 * rng.standard_normal((nq, dim)).astype(np.float32) / np.sqrt(dim)
    q[3] = rows[999]                       # hits the run of identical rows
    q[4] = rows[17]
    q[8, 3] = np.nan                       # non-finite queries cannot be certified: exact path, same bits
    q[9, 0] = np.inf
    q[10] *= 1e30                          # f16-overflowing query
    q[11] *= 1e-30                         # f16-subnormal / underflowing query
    allow = rng.random(n) > 0.5
    for k, mask in ((10, None), (64, None), (10, allow), (7, allow)):
        br, bs, bc, fb = idx.search_batched(q, k, allow=mask)
        er, es, ec = idx.search_batch(q, k, mask)
        assert np.array_equal(bc, ec) and np.array_equal(br, er) and np.array_equal(bits(bs), bits(es)), (k, mask is None)
        assert fb < nq // 4, fb
    br, bs, bc, _ = idx.search_batched(q, 10)
    for qi in (3, 4, 130, 199):
        orow, osc = oracle.search_top_k(slab, q[qi], 10)
        assert np.array_equal(br[qi], orow) and np.array_equal(bits(bs[qi]), bits(osc))


def test_config2_batched_1m_rows_against_the_oracle(fa, oracle, batched_filter):
    """BASELINE config 2: 1M x 384 f16 (the reference bench corpus, generated on the GPU), top-10, batches of 8 / 64 / 256
    queries through the batched matrix-core path (256 takes the register-resident-query main pass) — every hit of a spread of
    queries against the oracle, the rest against the exact kernels."""
    import ctypes as C
    import torch
    n, dim, k = 1_000_000, 384, 10
    slab_t = torch.empty((n, dim), dtype=torch.float16, device="cuda:0")
    fa._lib.lib().fsgpu_bench_fixture_device(0, 0, n, dim, 64, C.c_float(0.30), 1, 1, slab_t.data_ptr(), None)
    host = slab_t.view(torch.int16).cpu().numpy().view(np.uint16)
    assert np.array_equal(host[:2048], oracle.clustered_corpus_f16(0, 2048, dim))
    idx = fa.VectorIndex.from_device_slab(slab_t.data_ptr(), n, dim, device=0, keepalive=slab_t)
    q = np.stack([oracle.clustered_query(i, dim) for i in range(256)])
    for b in (8, 64, 256):
        br, bs, bc, fb = idx.search_batched(q[:b], k)
        assert np.all(bc == k) and fb <= b // 8
        er, es, _ = idx.search_batch(q[:min(b, 64)], k)
        assert np.array_equal(br[:min(b, 64)], er) and np.array_equal(bits(bs[:min(b, 64)]), bits(es))
        for qi in sorted({0, b // 2, b - 1}):
            orow, osc = oracle.search_top_k(host, q[qi], k, nthreads=8)
            assert np.array_equal(br[qi], orow) and np.array_equal(bits(bs[qi]), bits(osc)), (b, qi)


def test_mrl_batched_equals_per_query_and_oracle(fa, oracle):
    # fsgpu_search_mrl_batched = mrl_search (mrl.rs:241-395) for a batch: the truncated scan on the matrix cores over the
    # strided prefix view, one re-score launch; every hit (rows and score bits) against the per-query call and the oracle
    rng = np.random.default_rng(202)
    n, dim = 150_000, 384
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[:, :64] *= 3.0
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[700] = rows[33]                                   # exact duplicate: tie broken by the lower row
    slab = rows.astype(np.float16).view(np.uint16)
    live = rng.random(n) > 0.1
    idx = fa.VectorIndex.from_slab(slab, live=live)
    nq = 300                                               # one 256-query wide pass + a 64-query tail
    q = rows[rng.integers(0, n, nq)] + 0.1 * rng.standard_normal((nq, dim)).astype(np.float32)
    q[5] = 0.0
    for sd, rd, rt, k in ((64, 0, 0, 10), (128, 0, 0, 10), (256, 0, 0, 7), (64, 128, 40, 10), (128, 0, 64, 20)):
        br, bs, bc, fb = idx.mrl_search_batched(q, k, sd, rd, rt)
        assert fb < nq // 4, (sd, fb)
        for qi in list(range(0, nq, 29)) + [5, 255, 256, 299]:
            hits = idx.mrl_search(q[qi], k, sd, rd, rt)
            assert [h.index for h in hits] == br[qi, :bc[qi]].tolist(), (sd, rd, rt, k, qi)
            assert np.array_equal(bits([h.score for h in hits]), bits(bs[qi, :bc[qi]])), (sd, rd, rt, k, qi)
        for qi in (0, 131, 299):
            er, es = oracle.mrl_search(slab, q[qi], k, sd, rd, rt, live=live)
            assert br[qi, :bc[qi]].tolist() == er.tolist() and np.array_equal(bits(bs[qi, :bc[qi]]), bits(es)), (sd, qi)
    # shapes the batched path does not cover go query by query and still agree
    br, bs, bc, fb = idx.mrl_search_batched(q[:9], 10, 20, 0, 0)
    assert fb == 9
    for qi in range(9):
        hits = idx.mrl_search(q[qi], 10, 20)
        assert [h.index for h in hits] == br[qi, :bc[qi]].tolist()


def test_batched_certificate_edges_overflow_subnormals_and_near_duplicates(fa, oracle, batched_filter):
    """The batched path is exact only through its certificate (|a - s| <= delta, mfma_scan.hip header); the cases where the
    certificate cannot hold or cannot separate must end on the exact kernels and still return the oracle's bits:
      * finite queries with one or a few elements above 65504 (their f16 image is +-inf) — marked uncertifiable up front;
      * queries made of f16-subnormal / underflowing elements (approximate scores collapse to ~0);
      * a corpus with >= 5000 rows within 2 delta of the k-th score: the candidate pool (1024) overflows -> exact fallback."""
    rng = np.random.default_rng(123)
    n, dim, k = 120_000, 384, 10
    base = rng.standard_normal(dim).astype(np.float32)
    base /= np.linalg.norm(base)
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    # 6000 near-duplicates of `base`, spread over the slab: scores against base differ by ~1e-4, far inside 2 delta ~ 1e-3
    dup = rng.choice(n, 6000, replace=False)
    rows[dup] = base + (1e-4 * rng.standard_normal((6000, dim))).astype(np.float32)
    slab = rows.astype(np.float16).view(np.uint16)
    idx = fa.VectorIndex.from_slab(slab)
    nq = 300                                  # one 256-query wide pass + a 64-query tail
    q = rows[rng.integers(0, n, nq)] + (0.2 * rng.standard_normal((nq, dim))).astype(np.float32)
    q[0] = base                               # sits on the near-duplicate cluster: pool overflow
    q[1] = base * 3.0
    q[2, 5] = 70000.0                         # one element above the f16 range, the rest ordinary
    q[3] = q[3] * 1e3
    q[3, 7] = -1.0e5
    q[4] = (rng.standard_normal(dim) * 3e-6).astype(np.float32)     # every element an f16 subnormal
    q[5] = (rng.standard_normal(dim) * 1e-9).astype(np.float32)     # every element underflows to f16 zero
    q[6, ::2] = 2e-6                          # half subnormal, half ordinary
    q[257] = base                             # the same hard query in the tail group
    br, bs, bc, fb = idx.search_batched(q, k)
    er, es, ec = idx.search_batch(q, k)
    assert np.array_equal(bc, ec) and np.array_equal(br, er) and np.array_equal(bits(bs), bits(es))
    # q2, q3 (f16 overflow) at least; on the f16 filter also q0, q1, q257 (its pool of 1,024 overflows — the int8 filter's finish
    # re-scores up to 8,192 candidates and takes the 6,000 near-duplicates in its stride)
    assert fb >= (2 if batched_filter == "int8 filter" else 4), fb
    for qi in (0, 2, 3, 4, 5, 6, 257):
        orow, osc = oracle.search_top_k(slab, q[qi], k)
        assert np.array_equal(br[qi], orow) and np.array_equal(bits(bs[qi]), bits(osc)), qi
    # the int8 batched pass 1 is integer-exact: a pile of tied int8 scores at the threshold must not lose a candidate
    r8, s8, c8, _ = idx.search_int8_two_pass_batched(q[:260], k, 3)
    for qi in (0, 1, 7, 257):
        hits = idx.search_top_k_int8_two_pass(q[qi], k, 3)
        assert [h.index for h in hits] == r8[qi, :c8[qi]].tolist(), qi


@pytest.mark.gpu
def test_mrl_search_matches_oracle(fa, oracle, tmp_path):
    # VectorIndex::mrl_search (crates/frankensearch-index/src/mrl.rs:241-395): truncated scan over a strided prefix of
    # every row + rescore; rows and score bits must equal the oracle's for every MrlConfig shape
    rng = np.random.default_rng(101)
    n, dim = 30_011, 384
    rows = rng.standard_normal((n, dim)).astype(np.float32)
    rows[:, :64] *= 3.0                                   # Matryoshka-like: the leading dimensions carry the signal
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    rows[500] = rows[20]                                  # exact duplicate: tie broken by the lower row
    slab = rows.astype(np.float16).view(np.uint16)
    live = rng.random(n) > 0.1
    idx = fa.VectorIndex.from_slab(slab, live=live)
    for qi in range(4):
        q = rows[rng.integers(0, n)] + 0.1 * rng.standard_normal(dim).astype(np.float32)
        for sd, rd, rt, k in ((64, 0, 0, 10), (128, 0, 0, 10), (256, 0, 0, 7), (20, 0, 0, 10), (64, 200, 0, 10),
                              (128, 64, 0, 5), (64, 0, 500, 10), (8, 0, n, 10), (64, 0, 0, 1), (384, 0, 0, 10),
                              (999, 0, 0, 10)):
            er, es = oracle.mrl_search(slab, q, k, sd, rd, rt, live=live)
            hits, st = idx.mrl_search(q, k, sd, rd, rt, with_stats=True)
            assert [h.index for h in hits] == er.tolist(), (qi, sd, rd, rt, k)
            assert np.array_equal(bits([h.score for h in hits]), bits(es)), (qi, sd, rd, rt, k)
            assert st["fell_back_to_full"] == (sd >= dim)
            if sd < dim:
                assert st["scan_dims"] == sd and st["rescore_dims"] == max(sd, rd if 0 < rd <= dim else dim)
                assert st["candidates_rescored"] == min(rt if rt else 3 * k, int(live.sum()))
    assert idx.mrl_search(q, 0, 64) == []
    with pytest.raises(fa.InvalidConfig):
        idx.mrl_search(q, 10, 0)
    with pytest.raises(fa.DimensionMismatch):
        idx.mrl_search(q[:100], 10, 64)
    # FSVI file with resident WAL entries and a tombstone (mrl.rs:1162-1221)
    rows40 = [(f"doc-{i:03}", rng.standard_normal(40).astype(np.float32)) for i in range(200)]
    p = str(tmp_path / "mrl.fsvi")
    oracle.fsvi_write(p, [(d, v.tolist()) for d, v in rows40])
    g = fa.VectorIndex.open(p)
    o = oracle.Fsvi(p)
    wal = []
    for j in range(6):
        v = rng.standard_normal(40).astype(np.float32)
        g.append(f"new-{j}", v)
        wal.append(v)
    g.soft_delete(g.doc_id_at(17))
    oslab = o.slab()          # rows in file order (sorted by doc-id hash), as the GPU index holds them
    live2 = np.ones(200, bool)
    live2[17] = False
    for sd, k in ((8, 5), (16, 12), (24, 3), (16, 300)):
        q = rng.standard_normal(40).astype(np.float32)
        er, es = oracle.mrl_search(oslab, q, k, sd, live=live2, wal=wal)
        hits = g.mrl_search(q, k, sd)
        assert [h.index for h in hits] == er.tolist() and np.array_equal(bits([h.score for h in hits]), bits(es))
        assert all(h.doc_id is not None for h in hits if h.index < 200)


@pytest.mark.gpu
def test_4bit_two_pass_matches_oracle(fa, oracle, tmp_path):
    # search.rs:876-946; keep-all fixture (search.rs:2010-2053); slab packer simd.rs:2153-2215
    slab = oracle.encode_f32_to_f16(oracle.fixture_hashmix(300, 70))       # dim 70: generic path, partial last byte
    idx = fa.VectorIndex.from_slab(slab)
    for qi in range(8):
        q = np.array([(((qi * 7 + j * 3) % 11) / 11.0) - 0.5 for j in range(70)], dtype=np.float32)
        er, es = oracle.search_4bit_two_pass(slab, q, 10, 50)
        gh = idx.search_top_k_4bit_two_pass(q, 10, 50)
        assert [h.index for h in gh] == er.tolist() and np.array_equal(bits([h.score for h in gh]), bits(es))
        xr, _ = oracle.search_top_k(slab, q, 10)
        assert [h.index for h in gh] == xr.tolist()                       # keep-all == exact
    rng = np.random.default_rng(73)
    for n, dim in ((20_000, 384), (9_000, 256), (5_003, 128), (700, 512), (1_000, 24), (1_000, 33)):
        rows = rng.standard_normal((n, dim)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        rows[7] = rows[3]                                                  # tie: lower row first
        slab = rows.astype(np.float16).view(np.uint16)
        live = rng.random(n) > 0.07
        idx = fa.VectorIndex.from_slab(slab, live=live)
        for qi in range(3):
            q = rows[rng.integers(0, n)] + 0.2 * rng.standard_normal(dim).astype(np.float32)
            if qi == 2:
                q[5] = np.nan                                              # NaN query element quantises to 0
            for k, mult in ((10, 5), (1, 1), (10, 20), (7, 0), (40, 3), (10, 100)):
                er, es = oracle.search_4bit_two_pass(slab, q, k, mult, live=live)
                gh = idx.search_top_k_4bit_two_pass(q, k, mult)
                assert [h.index for h in gh] == er.tolist(), (n, dim, qi, k, mult)
                assert np.array_equal(bits([h.score for h in gh]), bits(es)), (n, dim, qi, k, mult)
    assert idx.search_top_k_4bit_two_pass(q, 0, 5) == []
    with pytest.raises(fa.DimensionMismatch):
        idx.search_top_k_4bit_two_pass(q[:5], 3, 5)
    # all-zero slab: scale 0, every nibble 0
    z = fa.VectorIndex.from_slab(np.zeros((100, 128), np.uint16))
    er, es = oracle.search_4bit_two_pass(np.zeros((100, 128), np.uint16), np.ones(128, np.float32), 5, 3)
    gh = z.search_top_k_4bit_two_pass(np.ones(128, np.float32), 5, 3)
    assert [h.index for h in gh] == er.tolist()


@pytest.mark.gpu
def test_int8_two_pass_batched_equals_per_query_and_oracle(fa, oracle):
    # the batched int8 pass 1 runs on the int8 MFMA: scores are exact integers, so every query must get exactly the
    # candidates — hence exactly the hits — of search_top_k_int8_two_pass (search.rs:514-661)
    rng = np.random.default_rng(107)
    for n, dim in ((150_001, 384), (60_000, 256), (40_000, 128)):
        cent = rng.standard_normal((24, dim)).astype(np.float32)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        rows = cent[rng.integers(0, 24, n)] + 0.3 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        rows[4000:4030] = rows[3999]                       # a run of identical rows: int8 AND f16 ties, row order decides
        slab = rows.astype(np.float16).view(np.uint16)
        live = rng.random(n) > 0.05
        idx = fa.VectorIndex.from_slab(slab, live=live)
        nq = 150
        q = cent[rng.integers(0, 24, nq)] + 0.3 * rng.standard_normal((nq, dim)).astype(np.float32) / np.sqrt(dim)
        q[2] = rows[3999]
        q[5] = 0.0                                         # all-zero query: every int8 score ties at 0
        q[6] *= 11.0
        q[7, 3] = np.nan
        for k, mult in ((10, 3), (10, 1), (1, 5), (20, 3), (7, 0), (30, 3), (25, 5)):   # up to 125 candidates
            br, bs, bc, fb = idx.search_int8_two_pass_batched(q, k, mult)
            assert fb < nq // 3, (n, dim, k, mult, fb)
            for qi in list(range(12)) + [64, 127, 128, 149]:
                hits = idx.search_top_k_int8_two_pass(q[qi], k, mult)
                assert [h.index for h in hits] == br[qi, :bc[qi]].tolist(), (n, dim, k, mult, qi)
                assert np.array_equal(bits([h.score for h in hits]), bits(bs[qi, :bc[qi]])), (n, dim, k, mult, qi)
        i8 = oracle.quantize_slab_i8(slab)
        br, bs, bc, _ = idx.search_int8_two_pass_batched(q, 10, 3)
        for qi in (0, 2, 6, 100):
            er, es = oracle.search_int8_two_pass(slab, q[qi], 10, 3, live=live, slab_i8=i8)
            assert np.array_equal(br[qi, :bc[qi]], er) and np.array_equal(bits(bs[qi, :bc[qi]]), bits(es)), (n, dim, qi)
    # shapes the matrix-core path does not cover fall back per query, same answers
    small = fa.VectorIndex.from_slab(slab[:3000])
    br, bs, bc, fb = small.search_int8_two_pass_batched(q[:9], 10, 3)
    assert fb == 9
    for qi in range(9):
        hits = small.search_top_k_int8_two_pass(q[qi], 10, 3)
        assert [h.index for h in hits] == br[qi, :bc[qi]].tolist()
    br, bs, bc, fb = idx.search_int8_two_pass_batched(q[:5], 50, 3)     # k * mult = 150 > 128 candidates
    assert fb == 5
    for qi in range(5):
        hits = idx.search_top_k_int8_two_pass(q[qi], 50, 3)
        assert [h.index for h in hits] == br[qi, :bc[qi]].tolist()


@pytest.mark.gpu
def test_4bit_two_pass_batched_equals_per_query_and_oracle(fa, oracle):
    # the batched 4-bit pass 1 (search.rs:876-946) runs the nibble levels through the int8 matrix-core pass: the nibble dot is
    # an exact integer, so every query must get exactly the candidates — hence the hits — of search_top_k_4bit_two_pass.
    # 4-bit scores tie in droves (15 levels): the row-order tie-break at the candidate cut is what this exercises.
    rng = np.random.default_rng(211)
    for n, dim in ((150_001, 384), (50_000, 128)):
        cent = rng.standard_normal((24, dim)).astype(np.float32)
        cent /= np.linalg.norm(cent, axis=1, keepdims=True)
        rows = cent[rng.integers(0, 24, n)] + 0.3 * rng.uniform(-1, 1, (n, dim)).astype(np.float32)
        rows /= np.linalg.norm(rows, axis=1, keepdims=True)
        rows[4000:4030] = rows[3999]
        slab = rows.astype(np.float16).view(np.uint16)
        live = rng.random(n) > 0.05
        idx = fa.VectorIndex.from_slab(slab, live=live)
        nq = 300                                               # a 256-query wide pass + a tail
        q = cent[rng.integers(0, 24, nq)] + 0.3 * rng.uniform(-1, 1, (nq, dim)).astype(np.float32)
        q[2] = rows[3999]
        q[5] = 0.0
        q[6] *= 11.0
        q[7, 3] = np.nan
        q[8] *= 1e-10                                          # max |q| <= 1e-9: pack_4bit_query's scale is 0, all levels 0
        for k, mult in ((10, 5), (10, 1), (1, 5), (7, 0), (25, 5)):
            br, bs, bc, fb = idx.search_4bit_two_pass_batched(q, k, mult)
            assert fb < nq // 3, (n, dim, k, mult, fb)
            for qi in list(range(12)) + [64, 255, 256, 299]:
                hits = idx.search_top_k_4bit_two_pass(q[qi], k, mult)
                assert [h.index for h in hits] == br[qi, :bc[qi]].tolist(), (n, dim, k, mult, qi)
                assert np.array_equal(bits([h.score for h in hits]), bits(bs[qi, :bc[qi]])), (n, dim, k, mult, qi)
        br, bs, bc, _ = idx.search_4bit_two_pass_batched(q, 10, 5)
        for qi in (0, 2, 6, 8, 100):
            er, es = oracle.search_4bit_two_pass(slab, q[qi], 10, 5, live=live)
            assert np.array_equal(br[qi, :bc[qi]], er) and np.array_equal(bits(bs[qi, :bc[qi]]), bits(es)), (n, dim, qi)
    small = fa.VectorIndex.from_slab(slab[:3000])              # not covered by the matrix-core path: per query, same answers
    br, bs, bc, fb = small.search_4bit_two_pass_batched(q[:9], 10, 5)
    assert fb == 9
    for qi in range(9):
        hits = small.search_top_k_4bit_two_pass(q[qi], 10, 5)
        assert [h.index for h in hits] == br[qi, :bc[qi]].tolist()


@pytest.mark.gpu
def test_fsvi_writer_bytes_equal_reference_layout_and_config1_roundtrip(fa, oracle, tmp_path):
    # VectorIndexWriter (lib.rs:3637-3672, 3752-3943): the product writer must emit exactly the bytes the oracle's
    # restatement of the reference writer does — duplicate doc ids keep insertion order (stable sort), ids of different
    # lengths, a compaction generation — and reject what the reference rejects.
    rng = np.random.default_rng(113)
    rows = [(f"doc-{(i * 7919) % 613:04d}" + ("x" * (i % 5)), rng.standard_normal(40).astype(np.float32)) for i in range(600)]
    rows[10] = (rows[3][0], rows[10][1])               # duplicate doc id: last write lands after the first
    rows[11] = ("", rows[11][1])                       # empty doc id is legal in v1
    p_ref, p_gpu = str(tmp_path / "ref.fsvi"), str(tmp_path / "gpu.fsvi")
    assert oracle.fsvi_write(p_ref, [(d, v.tolist()) for d, v in rows], "potion", "rev-1", 3) == 0
    fa.write_fsvi(p_gpu, rows, "potion", "rev-1", 3)
    assert open(p_ref, "rb").read() == open(p_gpu, "rb").read()
    for bad in (np.full(40, np.nan, np.float32), np.zeros(40, np.float32), np.full(40, 3e38, np.float32)):
        with pytest.raises(fa.InvalidConfig):
            fa.write_fsvi(str(tmp_path / "bad.fsvi"), [("a", bad)])
    with pytest.raises(fa.InvalidConfig):
        fa.write_fsvi(str(tmp_path / "bad.fsvi"), [("d" * 70000, rows[0][1])])
    # BASELINE config 1 in miniature: token-id docs -> Model2Vec pool on the GPU -> FSVI write -> reopen ->
    # exact top-10; every stage equal to the oracle pipeline
    vocab, dim, ndocs = 4096, 256, 3000
    table = np.fromfunction(lambda r, c: ((r * 0.1 + c * 0.01) % 1.7) - 0.8, (vocab, dim)).astype(np.float32)
    docs = [rng.integers(0, vocab, int(rng.integers(3, 40))).tolist() for _ in range(ndocs)]
    m = fa.Model2VecEmbedder(table)
    emb = m.embed_batch_token_ids(docs)
    want = np.stack([oracle.m2v_embed(table, d) for d in docs])
    assert np.array_equal(emb.view(np.uint32), want.view(np.uint32))
    named = [(f"doc-{i:05d}", emb[i]) for i in range(ndocs)]
    p1, p2 = str(tmp_path / "c1_gpu.fsvi"), str(tmp_path / "c1_ref.fsvi")
    fa.write_fsvi(p1, named, "potion-multilingual-128M", "a28f4ee", 0)
    assert oracle.fsvi_write(p2, [(d, v.tolist()) for d, v in named], "potion-multilingual-128M", "a28f4ee", 0) == 0
    assert open(p1, "rb").read() == open(p2, "rb").read()
    g, o = fa.VectorIndex.open(p1), oracle.Fsvi(p1)
    for qi in range(5):
        q = oracle.m2v_embed(table, rng.integers(0, vocab, 9).tolist())
        oh, os_ = o.search_top_k(q, 10)
        gh = g.search_top_k(q, 10)
        assert [(h.index, h.doc_id) for h in gh] == [(h[0], h[2]) for h in oh]
        assert np.array_equal(bits([h.score for h in gh]), bits(os_))


@pytest.mark.gpu
def test_edge_cases_of_the_batched_and_two_pass_entry_points(fa, oracle, batched_filter):
    # empty batches, k = 0, k > N, fully tombstoned and one-row indexes must behave like the per-query exact search
    rng = np.random.default_rng(127)
    dim = 128
    slab = rng.standard_normal((50, dim)).astype(np.float16).view(np.uint16)
    q = rng.standard_normal((5, dim)).astype(np.float32)
    idx = fa.VectorIndex.from_slab(slab)
    for fn in (idx.search_batched, lambda qq, k: idx.search_int8_two_pass_batched(qq, k, 3)):
        r, s, c, fb = fn(q[:0], 10)
        assert r.shape[0] == 0 and c.shape[0] == 0
        r, s, c, fb = fn(q, 0)
        assert c.tolist() == [0] * 5
        r, s, c, fb = fn(q, 60)                                   # k > N: everything, best first
        assert c.tolist() == [50] * 5
        for i in range(5):
            er, es = oracle.search_top_k(slab, q[i], 60)
            assert np.array_equal(r[i, :50], er)
    assert idx.search_top_k_4bit_two_pass(q[0], 60, 5) != [] and len(idx.search_top_k_4bit_two_pass(q[0], 60, 5)) == 50
    assert len(idx.mrl_search(q[0], 60, 64)) == 50
    dead = fa.VectorIndex.from_slab(slab, live=np.zeros(50, bool))
    assert dead.search_batched(q, 5)[2].tolist() == [0] * 5
    assert dead.search_int8_two_pass_batched(q, 5, 3)[2].tolist() == [0] * 5
    assert dead.mrl_search(q[0], 5, 64) == [] and dead.search_top_k_4bit_two_pass(q[0], 5, 5) == []
    one = fa.VectorIndex.from_slab(slab[:1])
    r, s, c, _ = one.search_batched(q, 3)
    assert c.tolist() == [1] * 5 and r[:, 0].tolist() == [0] * 5
    big = rng.standard_normal((40_000, dim)).astype(np.float16).view(np.uint16)
    live = np.zeros(40_000, bool)
    live[[5, 777, 39_999]] = True                               # three live rows in a slab the matrix-core path accepts
    sparse = fa.VectorIndex.from_slab(big, live=live)
    r, s, c, fb = sparse.search_batched(np.tile(q, (20, 1)), 10)
    assert c.tolist() == [3] * 100 and set(r[0, :3].tolist()) == {5, 777, 39_999}
    r8, s8, c8, _ = sparse.search_int8_two_pass_batched(np.tile(q, (20, 1)), 10, 3)
    assert c8.tolist() == [3] * 100 and np.array_equal(r8[:, :3], r[:, :3])


@pytest.mark.gpu
def test_selective_filter_scores_only_the_allowed_rows(fa, oracle):
    # try_gather_filtered (search.rs:1114-1180): allowed * 50 < rows -> only the allowed rows are read; the result must be
    # the one the masked full scan gives (same dot order, same (score, row) selection), tombstones included
    rng = np.random.default_rng(77)
    n, dim = 300_000, 384
    slab = rand_slab(rng, n, dim)
    slab[1000:1040] = slab[999]  # ties across allowed rows: the lower row wins
    q = rng.standard_normal((3, dim)).astype(np.float32)
    live = rng.random(n) > 0.1
    for allowed, k, want_gather in ((40, 10, True), (40, 64, True), (5000, 10, True), (5000, 300, True),
                                    (5999, 10, True), (6001, 10, False), (9000, 1000, False)):
        allow = np.zeros(n, bool)
        allow[rng.choice(n, allowed, replace=False)] = True
        if allowed == 40:
            allow[:] = False
            allow[990:1030] = True
        for lv in (None, live):
            idx = fa.VectorIndex.from_slab(slab, live=lv)
            rows, scores, counts = idx.search_batch(q, k, allow=allow)
            g, s = idx.filter_stats()
            eff = allow if lv is None else (allow & lv)
            cnt = int(eff.sum())
            assert (g, s) == ((1, 0) if cnt * 50 < n and cnt > 0 else (0, 1)), (allowed, cnt, g, s)
            if lv is None:
                assert (g == 1) == want_gather
            for qi in range(3):
                er, es = oracle.search_top_k(slab, q[qi], k, live=eff)
                m = int(counts[qi])
                assert m == len(er) == min(k, cnt)
                assert np.array_equal(rows[qi, :m], er) and np.array_equal(bits(scores[qi, :m]), bits(es))
                assert np.all(rows[qi, m:] == 0xFFFFFFFF)
            idx.close()
    # nothing allowed: the masked scan answers (empty result)
    idx = fa.VectorIndex.from_slab(slab)
    rows, scores, counts = idx.search_batch(q, 5, allow=np.zeros(n, bool))
    assert np.all(counts == 0) and idx.filter_stats() == (0, 1)
    idx.close()


@pytest.mark.gpu
def test_candidate_hash_filter_through_the_record_table(fa, oracle, tmp_path):
    # SearchFilter::candidate_hashes -> rows by binary search in the (hash, doc_id)-sorted record table
    # (gather_positions_for_hashes, search.rs:1146-1198), then the filtered search; duplicate doc ids share a hash run
    rng = np.random.default_rng(43)
    n, dim = 6000, 64
    ids = [f"doc-{i % 5800:05}" for i in range(n)]  # 200 duplicated ids
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    p = str(tmp_path / "h.fsvi")
    assert oracle.fsvi_write(p, [(ids[i], vecs[i].tolist()) for i in range(n)], "emb", "r1") == 0
    o = oracle.Fsvi(p)
    g = fa.VectorIndex.open(p)
    row_ids = [o.doc_id(r) for r in range(n)]
    for wanted in (["doc-00007", "doc-00100", "doc-05799", "doc-00007", "no-such-doc"],      # selective: gathered
                   [f"doc-{i:05}" for i in range(0, 5800, 3)]):                              # a third: masked scan
        hashes = [oracle.fnv1a64(w.encode()) for w in wanted]
        bm, matched = g.allow_bitmap_for_hashes(hashes)
        want_rows = np.array([rid in set(wanted) for rid in row_ids])
        assert matched == int(want_rows.sum())
        assert np.array_equal(np.unpackbits(bm.view(np.uint8), bitorder="little")[:n].astype(bool), want_rows)
        q = rng.standard_normal((2, dim)).astype(np.float32)
        rows, scores, counts = g.search_batch(q, 10, allow=bm)
        slab = np.array(o.slab())
        for qi in range(2):
            # the oracle's filtered scan over the same file (doc-id dedup is a search_top_k matter, not search_batch's)
            er, es = oracle.search_top_k(slab, q[qi], 10, live=want_rows)
            m = int(counts[qi])
            assert m == len(er) and np.array_equal(rows[qi, :m], er) and np.array_equal(bits(scores[qi, :m]), bits(es))
    g.close()



@pytest.mark.gpu
@pytest.mark.parametrize("dim", [7, 40, 100, 384])
def test_f32_quantized_fsvi_files_open_and_search_like_the_reference(fa, oracle, tmp_path, dim):
    # Quantization::F32 (lib.rs:203-208): dot_product_f32_bytes_f32 (simd.rs:581-702) — leftover chunks join the sum
    # AFTER the accumulators are combined, fused tail; served by the general path.  Writer bytes == the oracle writer's.
    rng = np.random.default_rng(100 + dim)
    n = 2500
    vecs = rng.standard_normal((n, dim)).astype(np.float32)
    vecs[17] = vecs[11]  # a tie: the lower row wins
    ids = [f"doc-{i % 2400:05}" for i in range(n)]  # 100 duplicated doc ids
    rows_in = [(ids[i], vecs[i].tolist()) for i in range(n)]
    pg, po = str(tmp_path / "g.fsvi"), str(tmp_path / "o.fsvi")
    fa.write_fsvi(pg, rows_in, "emb", "r1", compaction_gen=1, quantization=0)
    assert oracle.fsvi_write(po, rows_in, "emb", "r1", quantization=0) == 0
    assert open(pg, "rb").read() == open(po, "rb").read()
    o = oracle.Fsvi(po)
    g = fa.VectorIndex.open(pg)
    slab = np.frombuffer(open(po, "rb").read()[o.vectors_offset:], dtype="<f4").reshape(n, dim)
    q = rng.standard_normal((3, dim)).astype(np.float32)
    for k in (1, 10, 300, n + 5):
        rows, scores, counts = g.search_batch(q, k)
        for qi in range(3):
            er, es = oracle.search_top_k_f32(slab, q[qi], k)
            m = int(counts[qi])
            assert m == len(er) and np.array_equal(rows[qi, :m], er) and np.array_equal(bits(scores[qi, :m]), bits(es))
    # doc-id dedup + tombstones through search_top_k / soft_delete, against the oracle's file search
    for qi in range(3):
        oh, os_ = o.search_top_k(q[qi], 20)
        gh = g.search_top_k(q[qi], 20)
        assert [(h.index, h.doc_id) for h in gh] == [(h[0], h[2]) for h in oh]
        assert np.array_equal(bits([h.score for h in gh]), bits(os_))
    # filters: a selective one (gathered rows) and a broad one (masked scan)
    for allowed in (20, 1500):
        allow = np.zeros(n, bool)
        allow[rng.choice(n, allowed, replace=False)] = True
        rows, scores, counts = g.search_batch(q[:1], 10, allow=allow)
        er, es = oracle.search_top_k_f32(slab, q[0], 10, live=allow)
        assert np.array_equal(rows[0, :counts[0]], er) and np.array_equal(bits(scores[0, :counts[0]]), bits(es))
    # dot_query_at, the two-pass entry points (the reference falls back to the exact scan for F32, search.rs:579-585)
    # and the batched entry point all answer with the exact F32 result
    pick = rng.choice(n, 33, replace=False).astype(np.uint32)
    want = np.array([oracle.dot_f32_bytes_f32(slab[r], q[0]) for r in pick], np.float32)
    assert np.array_equal(bits(g.gather_dot(q[0], pick)), bits(want))
    exact = g.search_top_k(q[1], 10)
    for hits in (g.search_top_k_int8_two_pass(q[1], 10, 3), g.search_top_k_4bit_two_pass(q[1], 10, 5)):
        assert [(h.index, h.doc_id) for h in hits] == [(h.index, h.doc_id) for h in exact]
        assert np.array_equal(bits([h.score for h in hits]), bits([h.score for h in exact]))
    br, bs, bc, fb = g.search_batched(np.repeat(q, 30, axis=0), 10)
    for qi in range(3):
        e_r, e_s = oracle.search_top_k_f32(slab, q[qi], 10)
        assert np.array_equal(br[qi * 30], e_r) and np.array_equal(bits(bs[qi * 30]), bits(e_s))
    g.close()


@pytest.mark.gpu
def test_f32_fused_scan_at_scale_matches_the_oracle(fa, oracle, tmp_path):
    # scan_topk_f32_kernel (f32_kernels.hip): the fused scan + top-k of Quantization::F32 slabs — enough rows for every wave
    # to fill and compact its candidate buffer many times, ties, tombstones, a broad allow mask, k tiers up to the fused
    # limit (256) and beyond (general path), dims with and without leftover chunks (384 = 12 groups, 136 = 4 groups + 1 chunk)
    rng = np.random.default_rng(4242)
    for n, dim in ((120_000, 384), (90_001, 136)):
        vecs = rng.standard_normal((n, dim)).astype(np.float32)
        vecs[5000:5040] = vecs[4999]                       # a run of identical rows: the lower row wins
        vecs[n - 1] = vecs[4999]
        ids = [f"d{i:06}" for i in range(n)]
        path = str(tmp_path / f"big{dim}.fsvi")
        fa.write_fsvi(path, zip(ids, vecs), "emb", "r1", quantization=0)
        g = fa.VectorIndex.open(path)
        raw = open(path, "rb").read()
        off = oracle.Fsvi(path).vectors_offset
        slab = np.frombuffer(raw[off:], dtype="<f4").reshape(n, dim)   # file order (sorted by doc-id hash), as the index sees it
        q = rng.standard_normal((7, dim)).astype(np.float32)   # 7 queries: passes of 4, 2 and 1 (round 5: the kernel takes up to four per pass)
        q[1] = slab[4999] if np.array_equal(slab[4999], slab[5000]) else vecs[4999]
        allow = rng.random(n) > 0.4
        for k in (1, 10, 64, 256, 300):
            rows, scores, counts = g.search_batch(q, k)
            for qi in range(7):
                er, es = oracle.search_top_k_f32(slab, q[qi], k)
                m = int(counts[qi])
                assert m == len(er) and np.array_equal(rows[qi, :m], er) and np.array_equal(bits(scores[qi, :m]), bits(es)), (dim, k, qi)
        rows, scores, counts = g.search_batch(q, 10, allow=allow)
        for qi in range(7):
            er, es = oracle.search_top_k_f32(slab, q[qi], 10, live=allow)
            assert np.array_equal(rows[qi, :10], er) and np.array_equal(bits(scores[qi, :10]), bits(es)), (dim, qi)
        g.set_hreduce(2)
        rows, scores, counts = g.search_batch(q[:2], 10)
        for qi in range(2):
            er, es = oracle.search_top_k_f32(slab, q[qi], 10, hreduce=2)
            assert np.array_equal(rows[qi, :10], er) and np.array_equal(bits(scores[qi, :10]), bits(es)), (dim, qi)
        g.close()


@pytest.mark.gpu
def test_mrl_search_on_an_f32_index(fa, oracle, tmp_path):
    # mrl.rs:1700-1740 (mrl_search_f32_quantization): 16 dims, scan 8
    p = str(tmp_path / "m.fsvi")
    fa.write_fsvi(p, [("doc-a", [1.0] * 16), ("doc-b", [0.5] * 16)], "test", "mrl-test", quantization=0)
    g = fa.VectorIndex.open(p)
    hits, stats = g.mrl_search([1.0] * 16, 2, search_dims=8, rescore_dims=0, rescore_top_k=0, with_stats=True)
    assert [h.doc_id for h in hits] == ["doc-a", "doc-b"]
    assert stats["scan_dims"] == 8 and not stats["fell_back_to_full"]
    g.close()


@pytest.mark.gpu
def test_randomised_batched_cases_equal_the_per_query_kernels(fa):
    # scripts/fuzz_batched.py: random corpus shapes / data kinds (duplicates, few distinct rows, topical runs) /
    # tombstones / filters / ragged multi-group batches; 700 cases ran clean when this was added, a short slice runs here
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    res = subprocess.run([sys.executable, os.path.join(root, "scripts", "fuzz_batched.py"), "7", "12"], capture_output=True,
                         text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "0 mismatches" in res.stdout


@pytest.mark.gpu
def test_randomised_exact_cases_equal_the_oracle(fa, oracle):
    # tests/fuzz_exact.py: random sizes / dims (incl. unaligned) / k tiers / ties / outliers / tombstones / filters / F32
    # files against the oracle; 15,000 cases ran clean when this was added, a short slice runs here
    import subprocess
    import sys
    here = os.path.dirname(os.path.abspath(__file__))
    res = subprocess.run([sys.executable, os.path.join(here, "fuzz_exact.py"), "11", "10"], capture_output=True, text=True,
                         timeout=300)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "0 mismatches" in res.stdout


@pytest.mark.gpu
def test_reference_recall_fixture_on_the_gpu_paths(fa, oracle):
    # search.rs:1927-2006: on this corpus the int8 two-pass (multipliers 3 and 5) must reach recall@10 = 1.0 against the flat
    # search, for the first four centroids as queries; here additionally every path is held to the oracle's rows and bits
    cent, rows = oracle.recall_fixture()
    slab = oracle.encode_f32_to_f16(rows)
    idx = fa.VectorIndex.from_slab(slab)
    for c in range(4):
        q = cent[c]
        er, es = oracle.search_top_k(slab, q, 10)
        hits = idx.search_top_k(q, 10)
        assert [h.index for h in hits] == er.tolist() and np.array_equal(bits([h.score for h in hits]), bits(es))
        for mult in (3, 5):
            tr, ts = oracle.search_int8_two_pass(slab, q, 10, mult)
            th = idx.search_top_k_int8_two_pass(q, 10, mult)
            assert [h.index for h in th] == tr.tolist() and np.array_equal(bits([h.score for h in th]), bits(ts))
            assert set(tr.tolist()) == set(er.tolist()), (c, mult)          # recall@10 == 1.0, as the reference asserts
    # the batched forms over the same fixture (64 jittered queries): exact filter paths and the batched int8 two-pass
    q = np.stack([rows[i * 61] for i in range(64)])
    br, bs, bc, _ = idx.search_batched(q, 10)
    r8, s8, c8, _ = idx.search_int8_two_pass_batched(q, 10, 3)
    for qi in range(64):
        er, es = oracle.search_top_k(slab, q[qi], 10)
        assert np.array_equal(br[qi], er) and np.array_equal(bits(bs[qi]), bits(es)), qi
        tr, ts = oracle.search_int8_two_pass(slab, q[qi], 10, 3)
        assert np.array_equal(r8[qi, :c8[qi]], tr) and np.array_equal(bits(s8[qi, :c8[qi]]), bits(ts)), qi


def test_resident_allow_bitmap_gives_the_per_call_bitmaps_hits(fa, oracle):
    """fsgpu_allow_bitmap (a SearchFilter uploaded once, filter.rs:19-56): fsgpu_search_topk_filtered / _batched_filtered return the
    hits of the per-call bitmap — a broad filter (masked scan), a selective one (fewer than 1/50 of the rows: the gather of
    try_gather_filtered, search.rs:1114-1180), with tombstones that change AFTER the filter was made; the oracle agrees; concurrent
    single-query callers that share the handle ride one coalesced batch; a bitmap of another index is refused."""
    import threading
    rng = np.random.default_rng(77)
    n, dim = 120_077, 256
    slab = rand_slab(rng, n, dim)
    idx = fa.VectorIndex.from_slab(slab)
    q = rng.standard_normal((96, dim)).astype(np.float32)
    broad = rng.random(n) < 0.5
    narrow = rng.random(n) < 0.01
    for mask in (broad, narrow):
        f = idx.resident_filter(mask)
        assert f.allowed_rows() == int(mask.sum())
        for live in (None, rng.random(n) > 0.1):
            idx.set_live(live)
            a = idx.search_batch(q[:9], 10, allow=mask)
            b = idx.search_batch(q[:9], 10, allow=f)
            for x, y in zip(a, b):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
            orow, osc = oracle.search_top_k(slab, q[3], 10, live=mask if live is None else (mask & live))
            assert np.array_equal(b[0][3], orow) and np.array_equal(bits(b[1][3]), bits(osc))
            a = idx.search_batched(q, 10, allow=mask)
            b = idx.search_batched(q, 10, allow=f)
            for x, y in zip(a[:3], b[:3]):
                assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
        f.close()
    idx.set_live(None)
    # coalesced callers sharing one resident filter
    f = idx.resident_filter(broad)
    want = [idx.search_batch(q[i], 10, allow=f) for i in range(64)]
    idx.set_coalescing(64, 20_000)
    got, errs = [None] * 64, []

    def call(i):
        try:
            got[i] = idx.search_batch(q[i], 10, allow=f)
        except Exception as e:  # noqa: BLE001
            errs.append(e)

    ts = [threading.Thread(target=call, args=(i,)) for i in range(64)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert not errs, errs
    for i in range(64):
        for x, y in zip(got[i], want[i]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), i
    batches, requests = idx.coalescing_stats()
    assert requests == 64 and batches < 32
    idx.set_coalescing(0, 0)
    other = fa.VectorIndex.from_slab(slab[:1000])
    with pytest.raises(fa.InvalidConfig):
        other.search_batch(q[0], 5, allow=f)
    f.close()
    other.close()
    idx.close()


def test_profiling_period_times_every_nth_batched_step(fa):
    """fsgpu_index_set_profiling(n): of the batched search's main launches only those of every n-th call carry the HIP event pair
    (what bench.py times the dominant kernel with); answers are the same with and without."""
    rng = np.random.default_rng(5)
    n, dim = 150_016, 384
    slab = rand_slab(rng, n, dim)
    idx = fa.VectorIndex.from_slab(slab)
    q = rng.standard_normal((512, dim)).astype(np.float32)
    ref = idx.search_batched(q, 10)
    idx.scan_stats(reset=True)
    per_step = None
    for period, steps, timed in ((True, 6, 6), (4, 9, 3)):
        idx.set_profiling(period)
        for _ in range(steps):
            got = idx.search_batched(q, 10)
        idx.set_profiling(False)
        ms, launches, rows = idx.scan_stats(reset=True)
        if per_step is None:
            assert launches >= steps and launches % steps == 0, launches
            per_step = launches // steps
        assert launches == timed * per_step, (period, launches, per_step)
        assert ms > 0.0 and rows % n == 0 and rows >= launches * n
        for x, y in zip(ref[:3], got[:3]):
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32))
    idx.close()


def test_batched_search_in_two_halves_equals_the_blocking_call(fa):
    """fsgpu_search_topk_batched_device_begin / _end: a search begun while another is outstanding, ended in order, gives the blocking
    call's rows, score bits and counts (plain and packed outputs, with tombstones, queries the filter cannot certify included); a
    third begin is refused; a ticket ends once."""
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    from frankensearch_amd.errors import SearchError as FsgpuError
    rng = np.random.default_rng(9)
    n, dim = 180_011, 384
    slab = rand_slab(rng, n, dim)
    live = rng.random(n) > 0.05
    idx = fa.VectorIndex.from_slab(slab, live=live)
    dev = torch.device("cuda", 0)
    be = GpuShardBackend(idx, dev, batched=True)
    qs = []
    for j in range(5):
        q = rng.standard_normal((512 + 7 * j, dim)).astype(np.float32)
        q[3] = 0.0                      # an uncertifiable query: answered by the exact kernels in _end
        q[5, 0] = np.inf
        qs.append(torch.from_numpy(q).to(dev))
    want = [be.search_batched(q, 10) for q in qs]
    want_packed = [be.search_packed(q, 10) for q in qs]
    torch.cuda.synchronize()
    for packed in (False, True):
        got, prev = [], None
        for q in qs:
            cur = be.scan_begin(q, 10, packed=packed)
            if prev is not None:
                be.scan_end(prev[1])
                got.append(prev[0])
            prev = cur
        be.scan_end(prev[1])
        got.append(prev[0])
        torch.cuda.synchronize()
        for j in range(len(qs)):
            if packed:
                assert torch.equal(got[j], want_packed[j]), j
            else:
                for x, y in zip(got[j], want[j]):
                    assert torch.equal(x.view(torch.int32), y.view(torch.int32)), j
    a = be.scan_begin(qs[0], 10, packed=False)
    b = be.scan_begin(qs[1], 10, packed=False)
    with pytest.raises(FsgpuError):
        be.scan_begin(qs[2], 10, packed=False)
    # a blocking call in between is allowed (it queues behind the begun ones)
    r = be.search_batched(qs[2], 10)
    for x, y in zip(r, want[2]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    be.scan_end(a[1])
    be.scan_end(b[1])
    with pytest.raises(FsgpuError):
        be.scan_end(a[1])
    torch.cuda.synchronize()
    for x, y in zip(a[0], want[0]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    for x, y in zip(b[0], want[1]):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    idx.close()


def test_ticket_bookkeeping_at_the_edge_of_the_verdict_block(fa):
    """The pinned verdict block does not grow while a search is parked: with a 64-query search begun on a fresh index, a 600-query
    search — blocking or begun — is refused (INVALID_CONFIG, "... larger batch"), and the refused begin gives its ticket back: one more
    begin succeeds, the one after it is refused.  Both tickets end with the exact call's rows, score bits and counts, and once they
    have ended the 600-query search goes through."""
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    from frankensearch_amd.errors import InvalidConfig
    rng = np.random.default_rng(31)
    n, dim, k = 40_000, 128, 10          # just over the 32,768 rows the filters need
    slab = rand_slab(rng, n, dim)
    q = rng.standard_normal((600, dim)).astype(np.float32)
    twin = fa.VectorIndex.from_slab(slab)
    want = twin.search_batch(q, k, exact=True)   # fsgpu_search_topk_exact
    twin.close()
    idx = fa.VectorIndex.from_slab(slab)
    dev = torch.device("cuda", 0)
    be = GpuShardBackend(idx, dev, batched=True)
    qd = torch.from_numpy(q).to(dev)

    def assert_exact(got, lo, hi):
        torch.cuda.synchronize()
        r, s, c = (x.cpu().numpy() for x in got)
        assert np.array_equal(r.view(np.uint32), want[0][lo:hi]), (lo, hi)
        assert np.array_equal(bits(s), bits(want[1][lo:hi])), (lo, hi)
        assert np.array_equal(c.view(np.uint32), want[2][lo:hi]), (lo, hi)

    a = be.scan_begin(qd[:64], k, packed=False)          # parks: the verdict block is sized for 64 queries
    with pytest.raises(InvalidConfig, match="larger batch"):
        be.search_batched(qd, k)
    with pytest.raises(InvalidConfig, match="larger batch"):
        be.scan_begin(qd, k, packed=False)
    b = be.scan_begin(qd[64:96], k, packed=False)        # the refused begin released its ticket
    with pytest.raises(InvalidConfig, match="two begun batched searches are outstanding"):
        be.scan_begin(qd[96:128], k, packed=False)
    be.scan_end(a[1])
    be.scan_end(b[1])
    assert_exact(a[0], 0, 64)
    assert_exact(b[0], 64, 96)
    assert_exact(be.search_batched(qd, k), 0, 600)
    idx.close()


def test_end_half_refilters_through_the_nested_f16_batch_on_one_index(fa):
    """The corpus of test_queries_refiltered_in_the_end_half_travel_again (tests/test_gpu_sharded.py), its smallest parametrisation
    (90,000 x 256, noise 0.02, 4 clusters, 300 queries, k = 10), on ONE index with two tickets in flight: the int8 filter's lists
    overflow, and each ticket's END half hands more than 8 queries to the f16 filter as a nested batch (8 or fewer would take the
    fused exact pass instead).  late_answers is fallbacks + re-filtered, the hits are the exact call's bits, and both tickets'
    queries are accounted to the int8 filter."""
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    n, dim, noise, clusters, nq, k = 90_000, 256, 0.02, 4, 300, 10
    rng = np.random.default_rng(n + k)
    cent = rng.standard_normal((clusters, dim)).astype(np.float32)
    x = cent[rng.integers(0, clusters, n)] + (rng.standard_normal((n, dim)) * noise).astype(np.float32)
    x /= np.linalg.norm(x, axis=1, keepdims=True) + 1e-9
    slab = x.astype(np.float16).view(np.uint16)
    q = x[rng.integers(0, n, nq)] + (rng.standard_normal((nq, dim)) * 0.15).astype(np.float32)
    twin = fa.VectorIndex.from_slab(slab)
    want = [np.concatenate(z) for z in zip(*[twin.search_batch(q[s0:s0 + 64], k, exact=True) for s0 in range(0, nq, 64)])]
    twin.close()
    idx = fa.VectorIndex.from_slab(slab)
    dev = torch.device("cuda", 0)
    be = GpuShardBackend(idx, dev, batched=True)
    qd = torch.from_numpy(np.ascontiguousarray(q, dtype=np.float32)).to(dev)
    st0 = idx.batched_filter_stats()
    halves = [be.scan_begin(qd[:nq // 2], k, packed=False), be.scan_begin(qd[nq // 2:], k, packed=False)]
    fallbacks, late = [], []
    for _, ticket in halves:
        fallbacks.append(be.scan_end(ticket))
        late.append(be.last_late_answers)
    torch.cuda.synchronize()
    st1 = idx.batched_filter_stats()
    refiltered = st1["refiltered_f16"] - st0["refiltered_f16"]
    print(f"fallbacks {fallbacks}  late answers {late}  refiltered_f16 +{refiltered}  int8_queries +{st1['int8_queries'] - st0['int8_queries']}")
    assert refiltered > 0, "the case no longer re-filters: pick another corpus"
    for fb, la in zip(fallbacks, late):
        assert la - fb > 8, (fb, la)      # this ticket's re-filtered queries: the nested batch, not the fused exact pass
    assert sum(late) == sum(fallbacks) + refiltered
    got = [np.concatenate([h[0][j].cpu().numpy() for h in halves]) for j in range(3)]
    assert np.array_equal(got[0].view(np.uint32), want[0])
    assert np.array_equal(bits(got[1]), bits(want[1]))
    assert np.array_equal(got[2].view(np.uint32), want[2])
    assert st1["int8_queries"] - st0["int8_queries"] == nq
    idx.close()

"""GPU checks of the k-NN graph build (fsgpu_index_build_knn_graph / fsgpu_sharded_build_knn_graph): every list equals the index's own
row-level search with the self rule applied, and the CPU oracle's exact search — rows and similarity bits, no tolerance."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import smooth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = R.PAD


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)


def lists_from_hits(hit_rows, hit_scores, counts, sources, m):
    """The self rule over per-source top-(m + 1) answers -> ([n, m] rows, [n, m] sim bits)."""
    n = len(sources)
    rows = np.full((n, m), PAD, dtype=np.uint32)
    sims = np.zeros((n, m), dtype=F32)
    for i, src in enumerate(sources):
        c = int(counts[i])
        hr = [int(x) for x in hit_rows[i][:c]]
        kept = R.knn_from_topk(hr, int(src), m)
        score_of = {r: s for r, s in zip(hr, hit_scores[i][:c])}
        for x, r in enumerate(kept):
            if r != PAD:
                rows[i, x] = r
                sims[i, x] = score_of[r]
    return rows, sims


def expect_from_batched(idx, vectors_f32, sources, live, m):
    """search_batched(rows as f32, m + 1) of the same handle, self rule applied; tombstoned sources: padding."""
    sources = np.asarray(sources)
    alive = sources[live[sources]]
    want_rows = np.full((len(sources), m), PAD, dtype=np.uint32)
    want_sims = np.zeros((len(sources), m), dtype=F32)
    pos = {int(s): i for i, s in enumerate(sources)}
    for at in range(0, len(alive), 4096):
        part = alive[at:at + 4096]
        hr, hs, cnt, _ = idx.search_batched(vectors_f32[part], m + 1)
        r, s = lists_from_hits(hr, hs, cnt, part, m)
        where = [pos[int(x)] for x in part]
        want_rows[where], want_sims[where] = r, s
    return want_rows, want_sims


def expect_from_oracle(search, sources, live, m):
    """search(source) -> (rows, scores) of the CPU oracle's exact top-(m + 1)."""
    hit_rows, hit_scores, counts, kept = [], [], [], []
    for s in sources:
        if not live[s]:
            continue
        r, sc = search(int(s))
        hit_rows.append(r), hit_scores.append(sc), counts.append(len(r)), kept.append(int(s))
    return kept, lists_from_hits(hit_rows, hit_scores, counts, kept, m)


def assert_same(got_rows, got_sims, want_rows, want_sims, what):
    bad = np.flatnonzero((got_rows != want_rows).any(axis=1) | (bits(got_sims) != bits(want_sims)).any(axis=1))
    print(f"{what}: {got_rows.shape[0]} lists, differing {bad.size}")
    assert bad.size == 0, (what, bad[:5], got_rows[bad[:2]], want_rows[bad[:2]])


# ---- 1. the matrix path ----

def test_matrix_path_40000_by_64_with_tombstones_and_planted_duplicates(oracle):
    fa = _fa()
    rng = np.random.default_rng(64)
    n, dim, m = 40_000, 64, 10
    vec = unit_rows(rng, n, dim).astype(np.float16)
    planted = [17, 5_000, 12_345, 20_001, 33_333, 39_990]
    vec[planted] = vec[planted[0]]
    live = np.ones(n, dtype=bool)
    dead = rng.choice(np.setdiff1d(np.arange(n), planted), size=n // 100, replace=False)
    live[dead] = False
    live[planted[3]] = False                     # one copy is tombstoned
    idx = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
    wide = vec.astype(F32)
    before = idx.batched_filter_stats()
    rows, sims = idx.build_knn_graph(m, want_sims=True)
    after = idx.batched_filter_stats()
    print("int8 filter stats before / after the build:", before, after)
    assert after["int8_queries"] - before["int8_queries"] >= int(live.sum()), "the build did not ride the int8-filtered matrix path"
    assert rows.shape == (n, m) and sims.shape == (n, m)
    # tombstoned sources: padding; tombstoned rows: never a target
    assert (rows[~live] == PAD).all() and (bits(sims[~live]) == 0).all()
    assert not np.isin(rows[live], np.flatnonzero(~live)).any()
    assert not (rows == np.arange(n, dtype=np.uint32)[:, None]).any()
    # every source against the handle's own batched search
    want_rows, want_sims = expect_from_batched(idx, wide, np.arange(n), live, m)
    assert_same(rows, sims, want_rows, want_sims, "all sources vs search_batched")
    # 256 seeded sources + the planted rows against the CPU oracle
    sample = np.unique(np.concatenate([rng.choice(n, size=256, replace=False), planted]))
    slab = vec.view(np.uint16)
    kept, (orows, osims) = expect_from_oracle(lambda s: oracle.search_top_k(slab, wide[s], m + 1, live=live), sample, live, m)
    assert_same(rows[kept], sims[kept], orows, osims, "sample vs the oracle")
    # m = 3: the highest copy has four live lower-numbered copies in front of it, so it is absent from its own top 4
    for p in planted:
        r3 = idx.build_knn_graph(3, first_row=p, n_rows=1)
        if not live[p]:
            assert (r3 == PAD).all()
            continue
        hr, _, cnt, _ = idx.search_batched(wide[p][None, :], 4)
        assert r3[0].tolist() == R.knn_from_topk(hr[0][:int(cnt[0])], p, 3)
        if p == planted[-1]:
            assert p not in hr[0].tolist()
            assert r3[0].tolist() == planted[:3]
    idx.close()


def test_matrix_path_33000_by_384_a_slice_off_the_chunk_size(oracle):
    fa = _fa()
    rng = np.random.default_rng(384)
    n, dim, m = 33_000, 384, 10
    vec = unit_rows(rng, n, dim).astype(np.float16)
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, size=n // 100, replace=False)] = False
    idx = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
    first, count = 1_000, 2_500
    before = idx.batched_filter_stats()["int8_queries"]
    rows, sims = idx.build_knn_graph(m, first_row=first, n_rows=count, want_sims=True)
    assert idx.batched_filter_stats()["int8_queries"] > before
    sources = np.arange(first, first + count)
    wide = vec[first:first + count].astype(F32)
    full = np.zeros((n, dim), F32)
    full[first:first + count] = wide
    want_rows, want_sims = expect_from_batched(idx, full, sources, live, m)
    assert_same(rows, sims, want_rows, want_sims, "slice vs search_batched")
    sample = rng.choice(sources, size=256, replace=False)
    slab = vec.view(np.uint16)
    kept, (orows, osims) = expect_from_oracle(lambda s: oracle.search_top_k(slab, full[s], m + 1, live=live), sample, live, m)
    at = [k - first for k in kept]
    assert_same(rows[at], sims[at], orows, osims, "slice sample vs the oracle")
    idx.close()


# ---- 2. the general paths: every source against the oracle ----

def _check_f16_against_oracle(fa, oracle, vec, live, m, mode=None):
    idx = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live) if live is not None else None)
    n = vec.shape[0]
    live = np.ones(n, dtype=bool) if live is None else live
    mode = fa._lib.HREDUCE_SSE2 if mode is None else mode
    idx.set_hreduce(mode)
    rows, sims = idx.build_knn_graph(m, want_sims=True)
    slab, wide = vec.view(np.uint16), vec.astype(F32)
    kept, (orows, osims) = expect_from_oracle(lambda s: oracle.search_top_k(slab, wide[s], m + 1, live=live, hreduce=mode),
                                              np.arange(n), live, m)
    assert_same(rows[kept], sims[kept], orows, osims, f"{n} x {vec.shape[1]} f16, hreduce {mode}")
    assert (rows[~live] == PAD).all() and (bits(sims[~live]) == 0).all()
    idx.close()
    return rows


@pytest.mark.parametrize("dim,n", [(43, 2_500), (768, 1_203)])
def test_f16_general_dimensions_every_source_against_the_oracle(oracle, dim, n):
    fa = _fa()
    rng = np.random.default_rng(dim)
    vec = unit_rows(rng, n, dim).astype(np.float16)
    vec[n - 1] = vec[3]                      # a duplicate pair across the chunk boundary
    live = np.ones(n, dtype=bool)
    live[[5, n // 2, n - 2]] = False
    modes = (fa._lib.HREDUCE_SSE2, fa._lib.HREDUCE_SEQ) if dim == 43 else (fa._lib.HREDUCE_SSE2,)
    for mode in modes:
        _check_f16_against_oracle(fa, oracle, vec, live, 10, mode)


def test_f32_slab_of_wide_range_values_every_source_against_the_oracle(oracle, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(2100)
    n, dim, m = 1_203, 100, 10
    vec = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-7, 7, (n, 1))) * np.exp(rng.uniform(-2, 2, (n, dim)))).astype(F32)
    path = str(tmp_path / "wide100.fsvi")
    fa.write_fsvi(path, [(f"doc-{i:05d}", vec[i]) for i in range(n)], quantization=0)
    idx = fa.VectorIndex.open(path)
    stored = np.stack([idx.vector_at(r) for r in range(n)])      # file order: sorted by doc-id hash
    live = np.ones(n, dtype=bool)
    rows, sims = idx.build_knn_graph(m, want_sims=True)
    kept, (orows, osims) = expect_from_oracle(lambda s: oracle.search_top_k_f32(stored, stored[s], m + 1), np.arange(n), live, m)
    assert_same(rows[kept], sims[kept], orows, osims, "F32 slab 1,203 x 100")
    # with rows of very different norms a row is often not its own best hit: the self entry was found wherever it stood
    hr = [oracle.search_top_k_f32(stored, stored[s], m + 1)[0] for s in range(0, n, 7)]
    assert any(int(h[0]) != s for h, s in zip(hr, range(0, n, 7)))
    idx.close()


def test_padded_lists_one_row_and_all_but_one_tombstoned(oracle):
    fa = _fa()
    rng = np.random.default_rng(5)
    five = unit_rows(rng, 5, 64).astype(np.float16)
    rows = _check_f16_against_oracle(fa, oracle, five, None, 10)          # n = 5, m = 10: four entries and six pads
    assert ((rows != PAD).sum(axis=1) == 4).all() and (rows[:, 4:] == PAD).all()
    idx = fa.VectorIndex.from_slab(five[:1])
    r, s = idx.build_knn_graph(10, want_sims=True)                       # n = 1: one empty list
    assert r.shape == (1, 10) and (r == PAD).all() and (bits(s) == 0).all()
    # the errors that need a handle
    L = fa._lib.lib()
    out = np.zeros(64, np.uint32)
    for first, n in ((0, 2), (1, 1), (2, 0)):
        assert L.fsgpu_index_build_knn_graph(idx._h, first, n, 3, out.ctypes.data, None) == fa._lib.ERR_INVALID_CONFIG
    assert L.fsgpu_index_build_knn_graph(idx._h, 0, 1, 64, out.ctypes.data, None) == fa._lib.ERR_INVALID_CONFIG
    assert L.fsgpu_index_build_knn_graph(idx._h, 1, 0, 3, None, None) == 0
    idx.close()
    n = 300
    vec = unit_rows(rng, n, 128).astype(np.float16)
    live = np.zeros(n, dtype=bool)
    live[211] = True                                                     # all rows but one tombstoned
    idx = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
    r, s = idx.build_knn_graph(10, want_sims=True)
    assert (r == PAD).all() and (bits(s) == 0).all()
    idx.close()


# ---- 3. slices compose ----

def test_three_slices_concatenate_to_the_whole_graph():
    fa = _fa()
    rng = np.random.default_rng(33)
    n, dim, m = 2_500, 128, 7
    vec = unit_rows(rng, n, dim).astype(np.float16)
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, size=40, replace=False)] = False
    idx = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
    whole_rows, whole_sims = idx.build_knn_graph(m, want_sims=True)
    parts = [idx.build_knn_graph(m, first_row=a, n_rows=b, want_sims=True) for a, b in ((0, 1_000), (1_000, 37), (1_037, n - 1_037))]
    assert np.array_equal(np.concatenate([p[0] for p in parts]), whole_rows)
    assert np.array_equal(bits(np.concatenate([p[1] for p in parts])), bits(whole_sims))
    assert np.array_equal(idx.build_knn_graph(m), whole_rows)            # without the similarities: the same rows
    idx.close()


# ---- 4. sharded ----

def test_sharded_graph_equals_the_unsharded_table():
    fa = _fa()
    rng = np.random.default_rng(64)
    n, dim, m = 40_000, 64, 10
    vec = unit_rows(rng, n, dim).astype(np.float16)
    vec[[100, 15_000, 29_000]] = vec[100]                               # duplicates in three different shards
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, size=n // 100, replace=False)] = False
    whole = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
    want_rows, want_sims = whole.build_knn_graph(m, first_row=0, n_rows=3_000, want_sims=True)
    whole.close()
    for shards in (1, 2, 3):
        sh = fa.NativeShardedIndex.from_slab(vec, [0] * shards, live=fa.pack_bitmap(live), exchange=fa.NativeShardedIndex.EXCHANGE_PEER_COPY)
        got_rows, got_sims = sh.build_knn_graph(m, first_row=0, n_rows=3_000, want_sims=True)
        assert_same(got_rows, got_sims, want_rows, want_sims, f"{shards} shards vs unsharded")
        if shards == 3:   # a slice that starts in the last shard
            tail_rows = sh.build_knn_graph(m, first_row=n - 500, n_rows=500)
            one = fa.VectorIndex.from_slab(vec, live=fa.pack_bitmap(live))
            assert np.array_equal(tail_rows, one.build_knn_graph(m, first_row=n - 500, n_rows=500))
            one.close()
        sh.close()

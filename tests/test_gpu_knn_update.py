"""GPU checks of fsgpu_index_update_knn_graph / fsgpu_index_rewrite_sources: the updated table equals
fsgpu_index_build_knn_graph on the same handle AND knn_update_ref.update over the CPU oracle's exact scores — rows and similarity
bits, no tolerance — and the stats equal the reference's class counts.  At 20,000 rows and more the reference's lists are computed
for a seeded sample of every class (its classes and counts are always whole); the comparison with the handle's own build is always
over every row."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import knn_update_ref as U  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = U.PAD
COUNTS = ("rows", "dead", "added", "kept_clean", "kept_dirty", "searched_sources", "join_pairs", "rebuilt")


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)


def rewrite_map(rng, n0, drop, n_add, where="seeded"):
    """new_to_old of a rewrite that drops the old rows `drop` and inserts n_add rows (seeded places, all in front, or all behind)."""
    keep = np.setdiff1d(np.arange(n0), np.asarray(drop, dtype=np.int64))
    n1 = len(keep) + n_add
    new = np.zeros(n1, dtype=bool)
    new[{"seeded": rng.choice(n1, size=n_add, replace=False), "front": np.arange(n_add), "back": np.arange(len(keep), n1)}[where]] = True
    n2o = np.full(n1, PAD, dtype=np.uint32)
    n2o[~new] = keep
    return n2o


def apply_map(vec0, live0, n2o, add):
    vec1 = np.empty((len(n2o), vec0.shape[1]), dtype=vec0.dtype)
    live1 = np.ones(len(n2o), dtype=bool)
    old = n2o != PAD
    vec1[old], live1[old] = vec0[n2o[old]], live0[n2o[old]]
    if (~old).any():
        vec1[~old] = add
    return vec1, live1


def make_index(fa, vec, live, mode=0, row_base=0):
    make = fa.VectorIndex.from_slab_f32 if vec.dtype == np.float32 else fa.VectorIndex.from_slab
    idx = make(vec, live=None if live is None or live.all() else fa.pack_bitmap(live), row_base=row_base)
    idx.set_hreduce(mode)
    return idx


def oracle_fns(oracle, vec, live, mode):
    if vec.dtype == np.float32:
        def search(x, k):
            return oracle.search_top_k_f32(vec, vec[x], k, live=live, hreduce=mode)

        def score(x, rows):
            return np.array([oracle.dot_f32_bytes_f32(vec[int(r)], vec[x], mode) for r in rows], dtype=F32)
        return search, score
    slab, wide = np.ascontiguousarray(vec).view(np.uint16), vec.astype(F32)

    def search(x, k):
        return oracle.search_top_k(slab, wide[x], k, live=live, hreduce=mode)

    def score(x, rows):
        return oracle.gather_dot(slab, wide[x], np.asarray(rows, dtype=np.uint32), hreduce=mode)
    return search, score


def same_table(got, want_rows, want_bits, what, rows=None):
    g_rows, g_bits = got[0], U.bits_of(got[1]).reshape(got[0].shape)
    if rows is not None:
        g_rows, g_bits, want_rows, want_bits = g_rows[rows], g_bits[rows], want_rows[rows], want_bits[rows]
    bad = np.flatnonzero((g_rows != want_rows).any(axis=1) | (g_bits != want_bits).any(axis=1))
    print(f"{what}: {g_rows.shape[0]} lists, differing {bad.size}")
    assert bad.size == 0, (what, bad[:5], g_rows[bad[:2]], want_rows[bad[:2]])


def check_update(fa, oracle, idx1, old, n2o, vec1, live1, m, mode=0, frac=1.0, sample=None, old_row_base=0, row_base=0, join_covers=True,
                 what=""):
    """update on idx1 against its own build (every row) and against the reference (every row, or `sample` rows of each class)."""
    got_r, got_s, st = idx1.update_knn_graph(old[0], old[1], n2o, old_row_base=old_row_base, max_added_fraction=frac, want_stats=True)
    want_r, want_s = idx1.build_knn_graph(m, want_sims=True)
    same_table((got_r, got_s), want_r, U.bits_of(want_s).reshape(want_r.shape), what + " vs build_knn_graph")
    n = len(vec1)
    search, score = oracle_fns(oracle, vec1, live1, mode)
    sources = None
    if sample is not None:
        cls, _, _ = U.classify(old[0], U.bits_of(old[1]).reshape(old[0].shape), old_row_base, n2o, live1, n)
        rng = np.random.default_rng(n)
        sources = np.concatenate([rng.permutation(np.flatnonzero(cls == c))[:sample] for c in (U.DEAD, U.ADDED, U.CLEAN, U.DIRTY)])
    ref_r, ref_b, ref_st = U.update(old[0], old[1], n2o, live1, n, search, score, old_row_base=old_row_base, row_base=row_base,
                                    max_added_fraction=frac, join_covers=join_covers, sources=sources)
    same_table((got_r, got_s), ref_r, ref_b, what + " vs the reference", rows=sources)
    print(what, {k: st[k] for k in COUNTS + ("join_entries", "device_ms", "join_ms")})
    for k in COUNTS:
        assert st[k] == ref_st[k], (k, st[k], ref_st[k])
    if sources is None:
        assert st["join_entries"] == ref_st["join_entries"]
    else:   # the stat against the device's own output and the reference's classes
        is_added = np.append(cls == U.ADDED, False)
        local = np.where(got_r == PAD, n, got_r.astype(np.int64) - row_base)
        assert st["join_entries"] == int(is_added[local][cls == U.CLEAN].sum())
    return st


def evolve_and_check(fa, oracle, vec0, live0, n2o, add, m, mode=0, frac=1.0, sample=None, live1=None, what=""):
    idx0 = make_index(fa, vec0, live0, mode)
    old = idx0.build_knn_graph(m, want_sims=True)
    idx0.close()
    if n2o is None:
        vec1 = vec0
    else:
        vec1, carried = apply_map(vec0, live0, n2o, add)
        live1 = carried if live1 is None else live1
    idx1 = make_index(fa, vec1, live1, mode)
    st = check_update(fa, oracle, idx1, old, n2o, vec1, live1, m, mode, frac, sample, what=what)
    idx1.close()
    return st


# ---- 1. the exact path, F16, general dimensions, all three hreduce orders ----

@pytest.mark.parametrize("n,dim", [(2_500, 43), (1_203, 72)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_f16_general_dimensions_three_percent_dropped_two_percent_added(oracle, n, dim, mode):
    fa = _fa()
    rng = np.random.default_rng(n + dim)
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, rng.choice(n, size=n * 3 // 100, replace=False), n * 2 // 100)
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, unit_rows(rng, n * 2 // 100, dim), 10, mode, what=f"{n} x {dim} hreduce {mode}")
    assert st["rebuilt"] == 0 and st["join_pairs"] > 0 and st["searched_sources"] == st["added"] + st["kept_dirty"] and st["kept_dirty"] > 0


# ---- 2. the matrix path for the searched sources; two join blocks, the second of one row ----

def test_matrix_path_40000_by_64_with_1025_added_rows_tombstones_and_planted_duplicates(oracle):
    fa = _fa()
    rng = np.random.default_rng(64)
    n, dim, m = 40_000, 64, 10
    vec0 = unit_rows(rng, n, dim)
    planted = [17, 5_000, 12_345, 20_001, 33_333, 39_990]
    vec0[planted] = vec0[planted[0]]
    live0 = np.ones(n, dtype=bool)
    live0[rng.choice(np.setdiff1d(np.arange(n), planted), size=n // 100, replace=False)] = False
    live0[planted[3]] = False
    drop = rng.choice(np.setdiff1d(np.arange(n), planted), size=300, replace=False)
    n2o = rewrite_map(rng, n, drop, 1_025)
    add = unit_rows(rng, 1_025, dim)
    add[:3] = vec0[planted[0]]                 # three more copies arrive: they tie with the planted rows' entries
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, add, m, sample=40, what="40,000 x 64")
    assert st["rebuilt"] == 0 and st["added"] == 1_025 and st["join_pairs"] == st["kept_clean"] * 1_025 and st["dead"] > 0


# ---- 3. compile-time dimensions and group edges ----

def test_33000_by_384_with_17_added_rows_at_m_16(oracle):
    fa = _fa()
    rng = np.random.default_rng(384)
    n, dim, m = 33_000, 384, 16
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, rng.choice(n, size=20, replace=False), 17)       # 17: one over a 16-row chunk; 32,997 rows: a ragged tile
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, unit_rows(rng, 17, dim), m, sample=24, what="33,000 x 384")
    assert st["rebuilt"] == 0 and st["added"] == 17 and st["rows"] % 64 != 0


@pytest.mark.parametrize("m", [1, 63])
def test_1000_by_128_at_the_smallest_and_the_widest_list(oracle, m):
    fa = _fa()
    rng = np.random.default_rng(128 + m)
    n, dim = 1_000, 128
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, rng.choice(n, size=3, replace=False), 30)
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, unit_rows(rng, 30, dim), m, what=f"1,000 x 128 m {m}")
    assert st["rebuilt"] == 0 and st["kept_clean"] > 0 and st["rows"] % 64 != 0


@pytest.mark.parametrize("dim", [64, 256])
def test_the_other_compile_time_dimensions(oracle, dim):
    fa = _fa()
    rng = np.random.default_rng(dim)
    n = 700
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, [5, 600], 20)
    for mode in (0, 1, 2):
        st = evolve_and_check(fa, oracle, vec0, live0, n2o, unit_rows(rng, 20, dim), 10, mode, what=f"700 x {dim} hreduce {mode}")
        assert st["rebuilt"] == 0 and st["join_pairs"] > 0


# ---- 4. F32 slabs: leftovers after the tree, a fused tail ----

@pytest.mark.parametrize("dim", [40, 99])
def test_f32_slab_of_wide_range_values(oracle, dim):
    fa = _fa()
    rng = np.random.default_rng(2100 + dim)
    n, m = 1_500, 10

    def wide_rows(k):
        return (rng.standard_normal((k, dim)) * np.exp(rng.uniform(-7, 7, (k, 1))) * np.exp(rng.uniform(-2, 2, (k, dim)))).astype(F32)
    vec0, live0 = wide_rows(n), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, rng.choice(n, size=15, replace=False), 30)
    for mode in (0, 2):
        st = evolve_and_check(fa, oracle, vec0, live0, n2o, wide_rows(30), m, mode, what=f"F32 1,500 x {dim} hreduce {mode}")
        assert st["rebuilt"] == 0 and st["join_pairs"] > 0


# ---- 5. degenerate classes ----

def test_deletes_only_every_kept_row_dirty_every_row_added_and_short_lists(oracle):
    fa = _fa()
    rng = np.random.default_rng(5)
    vec0, live0 = unit_rows(rng, 900, 48), np.ones(900, dtype=bool)
    st = evolve_and_check(fa, oracle, vec0, live0, rewrite_map(rng, 900, [1, 450, 899], 0), None, 10, what="deletes only")
    assert st["added"] == 0 and st["join_pairs"] == 0 and st["join_entries"] == 0 and st["kept_dirty"] > 0 and st["kept_clean"] > 0
    # 24 rows at m = 20: a list names all but three of the others, so four dropped rows make every kept row dirty
    vec0, live0 = unit_rows(rng, 24, 48), np.ones(24, dtype=bool)
    st = evolve_and_check(fa, oracle, vec0, live0, rewrite_map(rng, 24, [0, 7, 8, 23], 2), unit_rows(rng, 2, 48), 20, what="all dirty")
    assert st["kept_clean"] == 0 and st["kept_dirty"] == 20 and st["added"] == 2 and st["rebuilt"] == 0
    # the old table of a one-row index: its only list is empty, so that row is added like the rest
    st = evolve_and_check(fa, oracle, vec0[:1], live0[:1], rewrite_map(rng, 1, [], 40, "back"), unit_rows(rng, 40, 48), 10, what="all added")
    assert st["added"] == 41 and st["kept_clean"] == 0 and st["kept_dirty"] == 0
    # 5 -> 12 rows at m = 10
    st = evolve_and_check(fa, oracle, vec0[:5], live0[:5], rewrite_map(rng, 5, [], 7), unit_rows(rng, 7, 48), 10, what="5 -> 12")
    assert st["added"] == 7 and st["kept_clean"] == 5


def test_identity_map_with_soft_deletes_and_rows_brought_back_by_set_live(oracle):
    fa = _fa()
    rng = np.random.default_rng(8)
    n, dim, m = 1_300, 43, 10
    vec = unit_rows(rng, n, dim)
    live0 = np.ones(n, dtype=bool)
    live0[[3, 640, 1_299]] = False
    idx = make_index(fa, vec, live0)
    old = idx.build_knn_graph(m, want_sims=True)
    live1 = live0.copy()
    live1[rng.choice(np.flatnonzero(live0), size=25, replace=False)] = False
    idx.set_live(live1)
    st = check_update(fa, oracle, idx, old, None, vec, live1, m, what="identity, soft deletes")
    assert st["added"] == 0 and st["dead"] == 28 and st["kept_dirty"] > 0
    old = idx.build_knn_graph(m, want_sims=True)
    live2 = live1.copy()
    live2[[3, 1_299]] = True
    live2[np.flatnonzero(~live1)[5:9]] = True
    idx.set_live(live2)
    st = check_update(fa, oracle, idx, old, None, vec, live2, m, what="identity, rows brought back")
    assert st["added"] == 6 and st["kept_dirty"] == 0 and st["join_pairs"] > 0
    idx.close()


# ---- 6. a tie at the m-th place, both ways ----

@pytest.mark.parametrize("where", ["front", "back"])
def test_an_added_twin_of_the_mth_entry_enters_only_with_the_lower_row(oracle, where):
    fa = _fa()
    rng = np.random.default_rng(33)
    n, dim, m = 80, 16, 3
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    twins = vec0[rng.choice(n, size=8, replace=False)].copy()
    n2o = rewrite_map(rng, n, [], 8, where)
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, twins, m, what=f"twins {where}")
    assert st["kept_dirty"] == 0 and st["kept_clean"] == n
    # the reference (equal to the device, above) shows both directions happen in this corpus: tests/test_knn_update_contract.py


# ---- 7. the fallbacks are the same table ----

def test_fallbacks_report_themselves_and_equal_the_build(oracle):
    fa = _fa()
    rng = np.random.default_rng(77)
    n, dim, m = 600, 64, 10
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    n2o = rewrite_map(rng, n, [9], 12)
    st = evolve_and_check(fa, oracle, vec0, live0, n2o, unit_rows(rng, 12, dim), m, frac=0.0, what="max_added_fraction 0")
    assert st["rebuilt"] == 2 and st["searched_sources"] == st["rows"] and st["join_pairs"] == 0
    perm = rng.permutation(n).astype(np.uint32)
    st = evolve_and_check(fa, oracle, vec0, live0, perm, None, m, what="a permuted map")
    assert st["rebuilt"] == 1 and st["kept_clean"] == 0 and st["searched_sources"] == n
    wide0 = unit_rows(rng, 150, 1_032)
    n2o = rewrite_map(rng, 150, [3], 4)
    idx0 = make_index(fa, wide0, None)
    old = idx0.build_knn_graph(m, want_sims=True)
    idx0.close()
    vec1, live1 = apply_map(wide0, np.ones(150, dtype=bool), n2o, unit_rows(rng, 4, 1_032))
    idx1 = make_index(fa, vec1, live1)
    st = check_update(fa, oracle, idx1, old, n2o, vec1, live1, m, join_covers=False, what="dimension 1,032")
    assert st["rebuilt"] == 3 and st["join_pairs"] == 0
    idx1.close()


# ---- 8. integration: FSVI, WAL, compact / vacuum, rewrite_sources ----

def _fsvi_index(fa, tmp_path, rng, n, dim):
    vec = unit_rows(rng, n, dim)
    path = str(tmp_path / "corpus.fsvi")
    fa.write_fsvi(path, [(f"doc-{i:06d}", vec[i].astype(F32)) for i in range(n)])
    idx = fa.VectorIndex.open(path)
    slab = np.stack([idx.vector_at(r) for r in range(n)]).astype(np.float16)       # file order: sorted by doc-id hash
    return idx, slab


def test_compaction_of_200_wal_entries_then_update(oracle, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(20_000)
    n, dim, m = 20_000, 64, 10
    idx, slab0 = _fsvi_index(fa, tmp_path, rng, n, dim)
    old = idx.build_knn_graph(m, want_sims=True)
    with pytest.raises(fa.InvalidConfig):
        idx.rewrite_sources()                                                      # no rewrite has happened on this handle
    fresh = unit_rows(rng, 200, dim)
    ids = [f"doc-{int(i):06d}" for i in rng.choice(n, size=100, replace=False)] + [f"new-{i:04d}" for i in range(100)]
    idx.append_batch([(d, fresh[i].astype(F32)) for i, d in enumerate(ids)])
    gen = idx.generation()
    idx.compact()
    n2o, before, after, old_n = idx.rewrite_sources()
    n1 = idx.record_count()
    assert (before, after, old_n) == (gen, gen + 1, n) and after == idx.generation() and n1 == n + 100 and n2o.shape == (n1,)
    slab1 = np.stack([idx.vector_at(r) for r in range(n1)]).astype(np.float16)
    kept = n2o != PAD
    assert (slab1[kept].view(np.uint16) == slab0[n2o[kept]].view(np.uint16)).all(), "a mapped row is not a copy of its old row"
    assert (np.diff(n2o[kept].astype(np.int64)) > 0).all() and int((~kept).sum()) == 200
    by_id = dict(zip(ids, fresh))
    for x in np.flatnonzero(~kept):
        assert (slab1[x].view(np.uint16) == by_id[idx.doc_id_at(int(x))].view(np.uint16)).all(), "a WAL-sourced row is not its WAL entry"
    live1 = np.ones(n1, dtype=bool)
    st = check_update(fa, oracle, idx, old, n2o, slab1, live1, m, sample=24, what="compact")
    assert st["rebuilt"] == 0 and st["added"] == 200 and st["kept_dirty"] > 0 and st["kept_clean"] > 15_000
    idx.close()


def test_soft_deletes_and_vacuum_then_update(oracle, tmp_path):
    fa = _fa()
    rng = np.random.default_rng(20_001)
    n, dim, m = 20_000, 64, 10
    idx, slab0 = _fsvi_index(fa, tmp_path, rng, n, dim)
    old = idx.build_knn_graph(m, want_sims=True)
    gone = [f"doc-{int(i):06d}" for i in rng.choice(n, size=150, replace=False)]
    dead_rows = {r for r in range(n) if idx.doc_id_at(r) in set(gone)}
    for d in gone:
        assert idx.soft_delete(d)
    idx.vacuum()
    n2o, before, after, old_n = idx.rewrite_sources()
    assert old_n == n and after == before + 1 and idx.record_count() == n - 150
    assert n2o.tolist() == [r for r in range(n) if r not in dead_rows]
    slab1 = slab0[n2o]
    st = check_update(fa, oracle, idx, old, n2o, slab1, np.ones(len(n2o), dtype=bool), m, sample=24, what="vacuum")
    assert st["rebuilt"] == 0 and st["added"] == 0 and st["kept_dirty"] > 0 and st["join_pairs"] == 0
    idx.close()


# ---- 9. refusals: the status, and nothing written ----

def test_refusals_leave_the_outputs_untouched():
    fa = _fa()
    rng = np.random.default_rng(1)
    n, dim, m = 50, 32, 4
    idx = make_index(fa, unit_rows(rng, n, dim), None)
    old_r, old_s = idx.build_knn_graph(m, want_sims=True)
    L = fa._lib.lib()
    out_r = np.full((n, m), 0xA5A5A5A5, dtype=np.uint32)
    out_s = np.full((n, m), 0xA5A5A5A5, dtype=np.uint32)
    ident = np.arange(n, dtype=np.uint32)
    p = lambda a: None if a is None else a.ctypes.data

    def call(m_=m, rows=old_r, sims=old_s, old_len=n, n2o=None, cfg=None, o_r=out_r, o_s=out_s):
        return L.fsgpu_index_update_knn_graph(idx._h, m_, p(rows), p(sims), old_len, 0, p(n2o), C.addressof(cfg) if cfg else None, p(o_r), p(o_s),
                                              None)
    bad_cfg = fa._lib.KnnUpdateConfig()
    bad_cfg.max_added_fraction = 1.0
    bad_cfg.reserved[3] = 1
    out_of_range, twice = ident.copy(), ident.copy()
    out_of_range[7] = n
    twice[8] = 9
    cases = {"m = 0": dict(m_=0), "m = 64": dict(m_=64), "no old rows": dict(rows=None), "no old sims": dict(sims=None),
             "no out rows": dict(o_r=None), "no out sims": dict(o_s=None), "old_len 2^32 - 1": dict(old_len=0xFFFFFFFF),
             "an entry that is neither the pad nor below old_len": dict(n2o=out_of_range), "one predecessor named twice": dict(n2o=twice),
             "identity with another old_len": dict(old_len=n - 1), "reserved words": dict(cfg=bad_cfg)}
    for why, kw in cases.items():
        assert call(**kw) == fa._lib.ERR_INVALID_CONFIG, why
        assert (out_r == 0xA5A5A5A5).all() and (out_s == 0xA5A5A5A5).all(), why
    # a begun search outstanding
    import torch
    q = torch.zeros((2, dim), dtype=torch.float32, device="cuda")
    o_rows = torch.zeros((2, 3), dtype=torch.int32, device="cuda")
    o_scores = torch.zeros((2, 3), dtype=torch.float32, device="cuda")
    o_counts = torch.zeros(2, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ticket = C.c_int32(-1)
    assert L.fsgpu_search_topk_batched_device_begin(idx._h, q.data_ptr(), 2, dim, 3, None, o_rows.data_ptr(), o_scores.data_ptr(),
                                                    o_counts.data_ptr(), None, None, C.byref(ticket)) == 0
    assert call() == fa._lib.ERR_INVALID_CONFIG and (out_r == 0xA5A5A5A5).all() and (out_s == 0xA5A5A5A5).all()
    assert L.fsgpu_search_topk_batched_device_end(idx._h, ticket.value, None) == 0
    # ... and the same arguments are accepted once it has ended
    assert call(n2o=ident) == 0 and (out_r == old_r).all() and (out_s == U.bits_of(old_s).reshape(n, m)).all()
    idx.close()
    empty = fa.VectorIndex.from_slab(np.zeros((0, dim), dtype=np.uint16))
    r, s = empty.update_knn_graph(np.zeros((0, m), np.uint32), np.zeros((0, m), F32))
    assert r.shape == (0, m) and s.shape == (0, m)
    empty.close()


# ---- 10. the join alone, one launch, between guard bands ----

# (dim 520: the workgroup drops to 2 waves, one leftover chunk before the tree; 1000: 1 wave, f16; 1003: 1 wave, f32, one leftover chunk
# after the tree and a fused tail of 3)
@pytest.mark.parametrize("dim,f32,mode", [(384, False, 0), (43, False, 2), (99, True, 0), (128, False, 1), (520, False, 0), (1000, False, 2),
                                          (1003, True, 1)])
def test_one_join_launch_over_tiles_that_mix_all_four_classes(oracle, dim, f32, mode):
    fa = _fa()
    rng = np.random.default_rng(dim)
    n, m, n_added = 203, 5, 21
    vec = (rng.standard_normal((n, dim)) * np.exp(rng.uniform(-3, 3, (n, 1)))).astype(F32) if f32 else unit_rows(rng, n, dim)
    cls = rng.integers(0, 4, size=n).astype(np.uint8)
    cls[:4] = [U.CLEAN, U.DEAD, U.ADDED, U.DIRTY]
    cls[64:128] = U.DIRTY                                    # a whole workgroup's tile without a kept-clean row
    added_rows = rng.permutation(np.flatnonzero(cls == U.ADDED))[:n_added].astype(np.uint32)
    added_rows.sort()
    others = np.flatnonzero(cls != U.ADDED)
    search, score = oracle_fns(oracle, vec, np.ones(n, dtype=bool), mode)
    # working table: every row holds a sorted list of 0 .. m entries over non-added rows with their true scores
    work_rows = np.full((n, m), PAD, dtype=np.uint32)
    work_bits = np.zeros((n, m), dtype=np.uint32)
    for x in range(n):
        have = rng.choice(others[others != x], size=int(rng.integers(0, m + 1)), replace=False)
        ent = U.order(list(zip((int(b) for b in U.bits_of(score(x, have))), (int(h) for h in have))))
        for c, (b, r) in enumerate(ent):
            work_rows[x, c], work_bits[x, c] = r, b
    want_rows, want_bits = U.join(work_rows, work_bits, cls, added_rows, score, m)
    packed = np.where(work_rows == PAD, np.uint64(0xFFFFFFFFFFFFFFFF), (work_bits.astype(np.uint64) << np.uint64(32)) | work_rows.astype(np.uint64))
    packed = np.ascontiguousarray(packed, dtype=np.uint64)
    block = np.ascontiguousarray(vec[added_rows].astype(F32))
    slab = np.ascontiguousarray(vec)
    status = fa._lib.lib().fsgpu_lab_knn_update_join(0, slab.ctypes.data, 1 if f32 else 0, n, dim, mode, m, cls.ctypes.data, packed.ctypes.data,
                                                     block.ctypes.data, added_rows.ctypes.data, len(added_rows))
    assert status == 0, fa._lib.lib().fsgpu_last_error()
    got_rows = np.where(packed == np.uint64(0xFFFFFFFFFFFFFFFF), PAD, packed & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    got_bits = np.where(packed == np.uint64(0xFFFFFFFFFFFFFFFF), 0, packed >> np.uint64(32)).astype(np.uint32)
    assert (got_rows == want_rows).all() and (got_bits == want_bits).all()
    untouched = cls != U.CLEAN
    assert (got_rows[untouched] == work_rows[untouched]).all() and (got_bits[untouched] == work_bits[untouched]).all()
    assert (got_rows[cls == U.CLEAN] != work_rows[cls == U.CLEAN]).any()

"""GPU checks of the graph ANN search (fsgpu_ann_*): the device returns the pure function of tests/ann_ref.py — rows, score bits, counts
and flags, no tolerance — over both corpora, both slab types, every hreduce order and the edges of every parameter; the answer does
not depend on the batch; refusals write nothing; certify_ef equals the reference certificate run on the device's own answers."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ann_ref as R  # noqa: E402
from ann_cases import assert_device_is_reference, bits, score_table, tombstones  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
PAD = R.PAD
N, M, NQ = 4096, 16, 33


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def make_case(fa, oracle, corpus, dim, f32, hreduce, seed, row_base=0):
    rng = np.random.default_rng(seed)
    if corpus == "iid":
        half = R.unit_rows(rng, N, dim).astype(np.float16)
        queries = R.unit_rows(rng, NQ, dim)
    else:
        half = oracle.clustered_corpus_f16(0, N, dim).view(np.float16)
        queries = np.stack([oracle.clustered_query(q, dim) for q in range(NQ)]).astype(F32)
    live = tombstones(rng, N)
    if f32:
        slab = (half.astype(F32) * F32(1.0009765625) + rng.standard_normal((N, dim)).astype(F32) * F32(1e-4)).astype(F32)   # not f16 values
        idx = fa.VectorIndex.from_slab_f32(slab, live=live, row_base=row_base)
    else:
        slab = half.view(np.uint16)
        idx = fa.VectorIndex.from_slab(slab, live=live, row_base=row_base)
    idx.set_hreduce(hreduce)
    table = idx.build_knn_graph(M)
    return idx, table, score_table(oracle, slab, queries, f32, hreduce), live, queries


# ---- 1. device == reference ----

@pytest.mark.parametrize("corpus,dim,f32,hreduce", [("iid", 64, False, 0), ("clustered", 384, False, 1), ("iid", 100, False, 2),
                                                    ("clustered", 64, True, 0), ("iid", 100, True, 1), ("iid", 384, True, 2)])
def test_device_is_the_reference(oracle, corpus, dim, f32, hreduce):
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, corpus, dim, f32, hreduce, seed=dim + hreduce)
    cfg = dict(n_entry=256)
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(**cfg))
    assert ann.record_count() == N and ann.device() == 0
    for k, ef in ((10, 64), (1, 16), (16, 16)):
        assert_device_is_reference(ann, table, scores, live, queries, k, ef, cfg, 0, f"{corpus} dim {dim} f32 {f32} hreduce {hreduce}")


def test_every_k_and_ef_and_every_parameter_edge(oracle):
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "iid", 64, False, 0, seed=11)
    cfg = dict(n_entry=256)
    ann = idx.build_ann(M, **cfg)   # build_knn_graph + fsgpu_ann_create: the same table
    for ef in (16, 64, 256):
        for k in (1, 10, ef):
            assert_device_is_reference(ann, table, scores, live, queries, k, ef, cfg, 0, "k / ef grid")
    # (expand 8 over 16 columns walks 128 rows a step: 32 steps reach the cap of 4,096 admitted rows)
    for cfg in (dict(n_entry=256, expand=1), dict(n_entry=256, expand=8, max_iters=32), dict(n_entry=256, max_iters=1),
                dict(n_entry=64, degree=8), dict(n_entry=N, max_iters=2), dict(n_entry=256, expand=8, degree=4)):
        ann = fa.AnnIndex(idx, table, fa.AnnConfig(**cfg))
        assert_device_is_reference(ann, table, scores, live, queries, 10, 64, cfg, 0, "parameter edge")
    cfg = dict(n_entry=1)   # the walk starts from row 0 alone
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(**cfg))
    assert_device_is_reference(ann, table, scores, live, queries, 10, 64, cfg, 0, "one entry row")


def test_row_base_is_added_to_every_row(oracle):
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "iid", 64, False, 0, seed=5, row_base=1000)
    assert table[live].min() >= 1000
    cfg = dict(n_entry=256)
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(**cfg))
    assert_device_is_reference(ann, table, scores, live, queries, 10, 64, cfg, 1000, "row_base 1000")


# ---- 2. against the exact search; batch invariance; the device form ----

def test_every_row_an_entry_row_is_the_exact_batched_search(oracle):
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "clustered", 384, False, 0, seed=3)
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(n_entry=N, max_iters=1))
    for k, ef in ((10, 10), (10, 256), (256, 256)):
        er, es, ec, _ = idx.search_batched(queries, k)
        rows, sc, counts, flags = ann.search_batched(queries, k, ef)
        assert (counts == ec).all() and (counts == k).all() and not flags.any()
        assert (rows == er).all() and (bits(sc) == bits(es)).all()


def test_an_answer_does_not_depend_on_the_batch_or_the_form(oracle):
    import torch
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "iid", 64, False, 0, seed=21)
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(n_entry=256))
    k, ef = 10, 32
    q = queries[7]
    r1, s1, flag = ann.search(q, k, ef)
    assert flag == 0 and r1.size == k
    rng = np.random.default_rng(0)
    batch = R.unit_rows(rng, 257, 64)
    for pos in (0, 100, 256):
        batch[pos] = q
    rows, sc, counts, flags = ann.search_batched(batch, k, ef)
    for pos in (0, 100, 256):
        assert counts[pos] == k and (rows[pos] == r1).all() and (bits(sc[pos]) == bits(s1)).all()
    dq = torch.from_numpy(batch).cuda()
    drows = torch.full((257, k), 7, dtype=torch.int32, device="cuda")
    dsc = torch.zeros((257, k), dtype=torch.float32, device="cuda")
    dcounts = torch.zeros(257, dtype=torch.int32, device="cuda")
    dflags = torch.full((257,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ann.search_batched_device(dq.data_ptr(), 257, k, ef, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
    assert (dcounts.cpu().numpy().view(np.uint32) == counts).all() and not dflags.cpu().numpy().any()
    assert (drows.cpu().numpy().view(np.uint32) == rows).all() and (bits(dsc.cpu().numpy()) == bits(sc)).all()


# ---- 3. the fallback ----

def test_underfilled_queries_are_answered_by_the_exact_search(oracle):
    import torch
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "iid", 64, False, 0, seed=31)
    nothing = np.full((N, M), PAD, dtype=np.uint32)
    live4 = np.ones(N, dtype=bool)
    idx.set_live(live4)
    ann = fa.AnnIndex(idx, nothing, fa.AnnConfig(n_entry=4))
    k = 10
    er, es, ec, _ = idx.search_batched(queries, k)
    rows, sc, counts, flags = ann.search_batched(queries, k, 16)
    assert (flags == R.UNDERFILLED).all() and (counts == ec).all() and (rows == er).all() and (bits(sc) == bits(es)).all()
    st = ann.stats
    assert (st.underfilled, st.approximate, st.rows_scored) == (NQ, 0, 4 * NQ)
    # k = 4 is filled by the four entry rows: approximate, and the best of those four
    rows, sc, counts, flags = ann.search_batched(queries[:3], 4, 16)
    assert not flags.any() and (counts == 4).all() and set(rows[0]) == {0, 1024, 2048, 3072}
    # all four entry rows tombstoned: count 0 with live rows left
    live4[[0, 1024, 2048, 3072]] = False
    idx.set_live(live4)
    er, es, ec, _ = idx.search_batched(queries, k)
    rows, sc, counts, flags = ann.search_batched(queries, k, 16)
    assert (flags == R.EMPTY_DESPITE_INDEXED_POINTS).all() and (rows == er).all() and (bits(sc) == bits(es)).all()
    # ... through the device form too
    dq = torch.from_numpy(queries).cuda()
    drows = torch.zeros((NQ, k), dtype=torch.int32, device="cuda")
    dsc = torch.zeros((NQ, k), dtype=torch.float32, device="cuda")
    dcounts = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    dflags = torch.zeros(NQ, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ann.search_batched_device(dq.data_ptr(), NQ, k, 16, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
    assert (dflags.cpu().numpy() == R.EMPTY_DESPITE_INDEXED_POINTS).all() and (dcounts.cpu().numpy() == k).all()
    assert (drows.cpu().numpy().view(np.uint32) == er).all() and (bits(dsc.cpu().numpy()) == bits(es)).all()
    # no live row at all: count 0 is the answer, nothing is flagged
    idx.set_live(np.zeros(N, dtype=bool))
    rows, sc, counts, flags = ann.search_batched(queries, k, 16)
    assert not counts.any() and not flags.any()


# ---- 4. refusals ----

def test_refusals_write_nothing(oracle):
    fa = _fa()
    idx, table, scores, live, queries = make_case(fa, oracle, "iid", 64, False, 0, seed=41)
    with pytest.raises(fa.InvalidConfig):
        fa.AnnIndex(idx, table[:-1], fa.AnnConfig())                      # graph_len != record_count
    for cfg in (dict(expand=9), dict(expand=0), dict(max_iters=0), dict(degree=17), dict(max_iters=65),    # 65 * 4 * 16 > 4,096
                dict(expand=8, max_iters=33), dict(n_entry=0)):
        with pytest.raises(fa.InvalidConfig):
            fa.AnnIndex(idx, table, fa.AnnConfig(**cfg))
    wide = np.full((N, 128), PAD, dtype=np.uint32)
    with pytest.raises(fa.InvalidConfig):
        fa.AnnIndex(idx, wide, fa.AnnConfig(expand=8, max_iters=1))       # 8 * 128 rows in one step
    big = fa.VectorIndex.from_slab(np.zeros((70_000, 8), dtype=np.uint16))
    with pytest.raises(fa.InvalidConfig):
        fa.AnnIndex(big, np.full((70_000, 1), PAD, dtype=np.uint32), fa.AnnConfig(n_entry=70_000))
    ann = fa.AnnIndex(idx, table, fa.AnnConfig(n_entry=256))
    L, C = fa._lib.lib(), __import__("ctypes")
    rows = np.full((NQ, 300), 0xABCDABCD, dtype=np.uint32)
    sc = np.full((NQ, 300), 7.0, dtype=F32)
    counts = np.full(NQ, 77, dtype=np.uint32)
    flags = np.full(NQ, 77, dtype=np.uint32)
    q = np.ascontiguousarray(queries)

    def call(nq, qlen, k, ef):
        return L.fsgpu_ann_search_batched(ann._h, q.ctypes.data, nq, qlen, k, ef, rows.ctypes.data, sc.ctypes.data, counts.ctypes.data,
                                          flags.ctypes.data, None)
    assert call(NQ, 64, 10, 9) == fa._lib.ERR_INVALID_CONFIG              # ef < k
    assert call(NQ, 64, 10, 257) == fa._lib.ERR_INVALID_CONFIG            # ef > 256
    assert call(NQ, 64, 0, 16) == fa._lib.ERR_INVALID_CONFIG              # k = 0
    assert call(NQ, 63, 10, 16) == fa._lib.ERR_DIMENSION_MISMATCH
    chosen, sweep, n = (C.c_byte * 16)(), (C.c_byte * 64)(), C.c_uint32(5)
    efs = np.asarray([16, 300], dtype=np.uint32)
    assert L.fsgpu_ann_certify_ef(ann._h, q.ctypes.data, NQ, efs.ctypes.data, 2, 10, 0.9, 0.1, chosen, sweep, C.byref(n)) == fa._lib.ERR_INVALID_CONFIG
    assert n.value == 5 and ann.stats.launches <= 1                        # refused before any launch
    # a vacuum that removes rows: the handle is stale
    assert idx.vacuum().tombstones_removed == int((~live).sum())
    assert call(NQ, 64, 10, 16) == fa._lib.ERR_INVALID_CONFIG and "stale" in fa._lib.last_error()
    assert (rows == 0xABCDABCD).all() and (sc == 7.0).all() and (counts == 77).all() and (flags == 77).all()
    with pytest.raises(fa.InvalidConfig):
        ann.certify_ef(queries, [16], 10, 0.9, 0.1)


# ---- 5. the certificate ----

def test_certify_ef_is_the_reference_certificate_on_the_devices_own_answers(oracle):
    fa = _fa()
    rng = np.random.default_rng(51)
    vec = R.unit_rows(rng, N, 64).astype(np.float16)
    idx = fa.VectorIndex.from_slab(vec.view(np.uint16))
    ann = idx.build_ann(M, n_entry=256)
    queries = R.unit_rows(rng, 200, 64)
    k, efs = 10, [16, 32, 64, 128]
    er, _, ec, _ = idx.search_batched(queries, k)
    asked = []

    def measure(ef):
        asked.append(ef)
        rows, _, counts, flags = ann.search_batched(queries, k, ef)
        return [R.recall_sample(rows[i, :counts[i]], flags[i], er[i, :ec[i]]) for i in range(len(queries))]
    for target in (0.3, 0.999):   # iid rows: a modest target certifies early, an extreme one never does
        asked.clear()
        want, want_sweep = R.calibrate(efs, measure, target, 0.1)
        chosen, sweep = ann.certify_ef(queries, [128, 16, 64, 32, 16], k, target, 0.1)
        st = ann.stats
        print(f"target {target}: chosen {chosen}, swept {[c.ef_search for c in sweep]}, launches {st.launches}, largest ef launched {st.ef_search}")
        assert (chosen.ef_search, chosen.certified_recall, chosen.meets_target) == want
        assert [(c.ef_search, c.certified_recall, c.meets_target) for c in sweep] == want_sweep
        assert st.launches == len(sweep) and st.ef_search == sweep[-1].ef_search and st.queries == 200 * len(sweep)
        if chosen.meets_target:
            assert st.ef_search == chosen.ef_search                          # no launch past the chosen ef
    assert [c.ef_search for c in sweep] == efs and not chosen.meets_target   # the extreme target swept them all

"""GPU checks of the IVF index (fsgpu_ivf_*): the device returns the pure functions of tests/ivf_ref.py bit for bit — centroid f32
bits, offsets and rows of a build; rows, score bits, counts and flags of a search — at the smallest shapes at which its kernels
can still go wrong; deletes made after the build are honoured; refusals write nothing; certify_nprobe equals the restated
certificate run on the device's own answers and ivf_ref's own choice."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ivf_cases as CS  # noqa: E402
import ivf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = R.bits


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


@functools.lru_cache(maxsize=None)
def hashmix_slab():
    from oracle import oracle
    oracle.build()
    return CS.f16(oracle.fixture_hashmix(4099, 64))


@functools.lru_cache(maxsize=None)
def big_slab():
    from oracle import oracle
    oracle.build()
    return oracle.clustered_corpus_f16(0, 20000, 384)


def assert_build_is_reference(ivf, want, what):
    cent = ivf.centroids()
    offsets, rows = ivf.lists()
    nan_d, nan_w = np.isnan(cent), np.isnan(want.centroids)
    assert (nan_d == nan_w).all(), f"{what}: NaN slots differ"
    same = (bits(cent) == bits(want.centroids)) | nan_w
    assert same.all(), f"{what}: {int((~same).sum())} centroid values differ, first at {np.argwhere(~same)[0]}"
    assert (offsets == want.offsets).all(), f"{what}: offsets differ"
    assert rows.size == want.rows.size and (rows == want.rows).all(), f"{what}: list rows differ"
    st = ivf.build_stats
    lens = np.diff(want.offsets.astype(np.int64))
    assert (st.rows_trained, st.rows_changed_last) == (want.trained, want.changed_last), what
    assert (st.empty_lists, st.largest_list, st.smallest_list) == (int((lens == 0).sum()), int(lens.max()), int(lens.min())), what


# ---- 1. build == ivf_ref ----

@pytest.mark.parametrize("nlist,iters,n_train,hreduce", [(16, 0, 0, 0), (17, 0, 0, 1), (16, 1, 0, 2), (17, 1, 1000, 0), (16, 3, 0, 1),
                                                         (17, 3, 1000, 2), (1, 1, 0, 0)])
def test_build_is_the_reference_on_the_hashmix_rows(oracle, nlist, iters, n_train, hreduce):
    fa = _fa()
    slab = hashmix_slab()
    live = CS.one_in_seven_dead(slab.shape[0])
    idx = fa.VectorIndex.from_slab(slab, live=live)
    idx.set_hreduce(hreduce)
    ivf = idx.build_ivf(nlist, iters=iters, n_train=n_train)
    assert (ivf.record_count(), ivf.nlist(), ivf.device(), ivf.build_stats.iterations) == (4099, nlist, 0, iters)
    want = R.build(oracle, slab, nlist, iters, n_train=n_train, live=live, hreduce=hreduce)
    assert_build_is_reference(ivf, want, f"nlist {nlist} iters {iters} n_train {n_train} hreduce {hreduce}")


@pytest.mark.parametrize("dim", [8, 72, 200])
def test_build_is_the_reference_at_the_join_tiles_odd_dimensions(oracle, dim):
    fa = _fa()
    slab = CS.normal_rows(dim, 1000, dim)
    idx = fa.VectorIndex.from_slab(slab)
    for hreduce in (0, 1, 2):
        idx.set_hreduce(hreduce)
        ivf = idx.build_ivf(19, iters=2)
        assert_build_is_reference(ivf, R.build(oracle, slab, 19, 2, hreduce=hreduce), f"dim {dim} hreduce {hreduce}")


def test_build_is_the_reference_over_several_tiles_and_chunks(oracle):
    fa = _fa()
    slab = big_slab()
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(64, iters=2)
    assert_build_is_reference(ivf, R.build(oracle, slab, 64, 2), "20,000 x 384")
    st = ivf.build_stats
    print(f"20,000 x 384, nlist 64, iters 2: assign {st.assign_ms:.3f} ms, update {st.update_ms:.3f} ms, lists {st.lists_ms:.3f} ms")


def test_build_takes_the_callers_centroids(oracle):
    fa = _fa()
    slab = hashmix_slab()
    init = np.random.default_rng(23).standard_normal((16, 64)).astype(F32)
    idx = fa.VectorIndex.from_slab(slab)
    for iters in (0, 2):
        ivf = idx.build_ivf(16, iters=iters, init_centroids=init)
        assert_build_is_reference(ivf, R.build(oracle, slab, 16, iters, init=init), f"caller's centroids, iters {iters}")
    assert (bits(idx.build_ivf(16, iters=0, init_centroids=init).centroids()) == bits(init)).all()


def test_ties_go_to_the_lower_centroid_and_an_empty_list_keeps_its_bits(oracle):
    fa = _fa()
    slab, nlist = CS.duplicate_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    offsets, _ = idx.build_ivf(nlist, iters=0).lists()
    lens = np.diff(offsets.astype(np.int64))
    assert (lens[1::2] == 0).all() and (lens[0::2] == 50).all()
    init = R.strided_init(slab, R.training_rows(slab.shape[0], 0), nlist)
    for iters in (0, 1, 2):
        ivf = idx.build_ivf(nlist, iters=iters)
        assert_build_is_reference(ivf, R.build(oracle, slab, nlist, iters), f"duplicates, iters {iters}")
    assert (bits(idx.build_ivf(nlist, iters=1).centroids()[1::2]) == bits(init[1::2])).all()


def test_non_finite_rows_follow_the_order_and_leave_their_centroids(oracle):
    fa = _fa()
    slab, nlist = CS.nonfinite_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    for iters in (0, 1, 2):
        ivf = idx.build_ivf(nlist, iters=iters)
        assert_build_is_reference(ivf, R.build(oracle, slab, nlist, iters), f"non-finite rows, iters {iters}")
    # a non-finite row as a centroid (the strided init may take one): NaN slots compare by NaN-ness
    init_rows = R.training_rows(slab.shape[0], 0)[(np.arange(120) * slab.shape[0]) // 120]
    assert 5 in init_rows and 40 in init_rows
    ivf = idx.build_ivf(120, iters=1)
    assert_build_is_reference(ivf, R.build(oracle, slab, 120, 1), "non-finite centroids")


def test_the_sequential_sum_is_kept_where_the_order_reaches_the_result(oracle):
    fa = _fa()
    slab, one = CS.cancelling_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(one, iters=1)
    assert_build_is_reference(ivf, R.build(oracle, slab, one, 1), "cancelling sums")
    print(f"a list of {slab.shape[0]} rows x 8: update {ivf.build_stats.update_ms:.3f} ms")


# ---- 2. search == ivf_ref.search ----

KS = (1, 10, 64, 65, 256)


@functools.lru_cache(maxsize=None)
def search_case(which):
    from oracle import oracle
    oracle.build()
    fa = _fa()
    if which == "hashmix":
        slab, nlist, live = hashmix_slab(), 16, CS.one_in_seven_dead(4099)
    else:
        slab, nlist, live = big_slab(), 64, None
    dim = slab.shape[1]
    idx = fa.VectorIndex.from_slab(slab, live=live, row_base=1000 if which == "hashmix" else 0)
    ivf = idx.build_ivf(nlist, iters=2)
    want = R.build(oracle, slab, nlist, 2, live=live)
    rng = np.random.default_rng(dim)
    queries = (R.widen(slab[rng.choice(slab.shape[0], 257, replace=False)]) + 0.1 * rng.standard_normal((257, dim))).astype(F32)
    return fa, idx, ivf, slab, want, queries, CS.score_table(oracle, slab, queries), live


@pytest.mark.parametrize("which", ["hashmix", "big"])
@pytest.mark.parametrize("nprobe", [1, 2, 5, "nlist"])
def test_search_is_the_reference(oracle, which, nprobe):
    fa, idx, ivf, slab, want, queries, table, live = search_case(which)
    assert_build_is_reference(ivf, want, which)
    nlist = ivf.nlist()
    nprobe = nlist if nprobe == "nlist" else nprobe
    row_base = 1000 if which == "hashmix" else 0
    scored = sum(R.rows_scored(oracle, want, q, nprobe) for q in queries)
    for k in KS:
        rows, sc, counts, flags = ivf.search_batched(queries, k, nprobe)
        st = ivf.stats
        bad, flagged = [], [0, 0, 0]
        for i, q in enumerate(queries):
            wr, ws, wf = R.search(oracle, slab, want, q, k, nprobe, row_base=row_base, row_scores=table[i],
                                  exact=CS.exact_from_scores(table[i]))
            flagged[wf] += 1
            if not (counts[i] == wr.size and flags[i] == wf and (rows[i, :wr.size] == wr).all() and (bits(sc[i, :wr.size]) == bits(ws)).all()):
                bad.append(i)
        assert not bad, f"{which} k {k} nprobe {nprobe}: queries {bad[:8]} differ"
        assert (st.approximate, st.underfilled, st.empty_despite_indexed_points) == tuple(flagged)
        assert (st.queries, st.nprobe, st.k_requested, st.nlist, st.lists_probed, st.rows_scored) == (257, nprobe, k, nlist, 257 * nprobe, scored)
        if nprobe == nlist:   # every list probed: the exact search
            er, es, ec = idx.search_batch(queries, k, exact=True)
            assert (counts == ec).all() and not flags.any()
            for i in range(257):
                assert (rows[i, :ec[i]] == er[i, :ec[i]]).all() and (bits(sc[i, :ec[i]]) == bits(es[i, :ec[i]])).all()


@pytest.mark.parametrize("which", ["hashmix", "big"])
def test_an_answer_does_not_depend_on_the_batch_or_the_form(oracle, which):
    import torch
    fa, idx, ivf, slab, want, queries, table, live = search_case(which)
    k, nprobe = 10, 5
    q = queries[7]
    r1, s1, flag = ivf.search(q, k, nprobe)
    assert flag == 0 and r1.size == k
    batch = queries.copy()
    for pos in (0, 128, 256):
        batch[pos] = q
    rows, sc, counts, flags = ivf.search_batched(batch, k, nprobe)
    for pos in (0, 128, 256):
        assert counts[pos] == k and (rows[pos] == r1).all() and (bits(sc[pos]) == bits(s1)).all()
    dq = torch.from_numpy(batch).cuda()
    drows = torch.full((257, k), 7, dtype=torch.int32, device="cuda")
    dsc = torch.zeros((257, k), dtype=torch.float32, device="cuda")
    dcounts = torch.zeros(257, dtype=torch.int32, device="cuda")
    dflags = torch.full((257,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ivf.search_batched_device(dq.data_ptr(), 257, k, nprobe, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
    assert (dcounts.cpu().numpy().view(np.uint32) == counts).all() and not dflags.cpu().numpy().any()
    assert (drows.cpu().numpy().view(np.uint32) == rows).all() and (bits(dsc.cpu().numpy()) == bits(sc)).all()


@pytest.mark.parametrize("nq,nprobe", [(15, 63), (16, 63), (16, 64), (15, 64)])
def test_both_coarse_steps_give_the_reference(oracle, nq, nprobe):
    """The coarse step is the centroid index's batched search below 16 queries or above 63 probes, the transposed join otherwise."""
    fa, idx, ivf, slab, want, queries, table, live = search_case("big")
    k = 10
    rows, sc, counts, flags = ivf.search_batched(queries[:nq], k, nprobe)
    for i in range(nq):
        wr, ws, wf = R.search(oracle, slab, want, queries[i], k, nprobe, row_scores=table[i], exact=CS.exact_from_scores(table[i]))
        assert counts[i] == wr.size and flags[i] == wf and (rows[i] == wr).all() and (bits(sc[i]) == bits(ws)).all(), (nq, nprobe, i)
    assert ivf.stats.rows_scored == sum(R.rows_scored(oracle, want, q, nprobe) for q in queries[:nq])


# ---- 3. deletes after the build, the fallback ----

def test_deletes_after_the_build_are_honoured_and_short_lists_fall_back(oracle):
    import torch
    fa = _fa()
    slab, init, query, short = CS.underfill_corpus()
    n = slab.shape[0]
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(2, iters=1, init_centroids=init)
    want = R.build(oracle, slab, 2, 1, init=init)
    assert_build_is_reference(ivf, want, "underfill corpus")
    other = R.widen(slab[3])
    queries = np.stack([query, other, query])
    k = 10
    # a probed list of 3 rows at k = 10: UNDERFILLED, answered by the exact search
    rows, sc, counts, flags = ivf.search_batched(queries, k, 1)
    er, es, ec = idx.search_batch(queries, k, exact=True)
    assert flags.tolist() == [R.UNDERFILLED, 0, R.UNDERFILLED] and (counts == k).all()
    assert (rows == er).all() and (bits(sc) == bits(es)).all()
    for i, q in enumerate(queries):
        wr, ws, wf = R.search(oracle, slab, want, q, k, 1)
        assert wf == flags[i] and (rows[i] == wr).all() and (bits(sc[i]) == bits(ws)).all()
    st = ivf.stats
    assert (st.underfilled, st.empty_despite_indexed_points, st.approximate, st.rows_scored) == (2, 0, 1, 3 + (n - 3) + 3)
    # one of the three deleted after the build: the old lists, the live bitmap of NOW
    live = np.ones(n, dtype=bool)
    live[short[0]] = False
    idx.set_live(live)
    r2, s2, flag = ivf.search(query, 2, 1)
    wr, ws, wf = R.search(oracle, slab, want, query, 2, 1, live_now=live)
    assert flag == wf == 0 and (r2 == wr).all() and (bits(s2) == bits(ws)).all() and sorted(r2.tolist()) == short[1:].tolist()
    # the probed list wholly dead: the exact answer, flagged EMPTY_DESPITE_INDEXED_POINTS — through both forms
    live[short] = False
    idx.set_live(live)
    rows, sc, counts, flags = ivf.search_batched(queries, k, 1)
    er, es, ec = idx.search_batch(queries, k, exact=True)
    assert flags.tolist() == [R.EMPTY, 0, R.EMPTY] and (rows == er).all() and (bits(sc) == bits(es)).all() and (counts == k).all()
    wr, ws, wf = R.search(oracle, slab, want, query, k, 1, live_now=live)
    assert wf == R.EMPTY and (rows[0] == wr).all() and (bits(sc[0]) == bits(ws)).all()
    st = ivf.stats
    assert (st.underfilled, st.empty_despite_indexed_points, st.approximate) == (0, 2, 1)
    dq = torch.from_numpy(queries).cuda()
    drows = torch.zeros((3, k), dtype=torch.int32, device="cuda")
    dsc = torch.zeros((3, k), dtype=torch.float32, device="cuda")
    dcounts = torch.zeros(3, dtype=torch.int32, device="cuda")
    dflags = torch.zeros(3, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ivf.search_batched_device(dq.data_ptr(), 3, k, 1, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
    assert dflags.cpu().numpy().tolist() == [R.EMPTY, 0, R.EMPTY] and (dcounts.cpu().numpy() == k).all()
    assert (drows.cpu().numpy().view(np.uint32) == er).all() and (bits(dsc.cpu().numpy()) == bits(es)).all()
    # no live row at all: count 0 is the answer, nothing is flagged
    idx.set_live(np.zeros(n, dtype=bool))
    rows, sc, counts, flags = ivf.search_batched(queries, k, 2)
    assert not counts.any() and not flags.any()


# ---- 4. refusals ----

def test_refusals_write_nothing(oracle, tmp_path):
    fa = _fa()
    slab = hashmix_slab()
    live = CS.one_in_seven_dead(4099)
    idx = fa.VectorIndex.from_slab(slab, live=live)
    with pytest.raises(fa.InvalidConfig):
        fa.VectorIndex.from_slab_f32(R.widen(slab)).build_ivf(16)                    # an F32 index
    with pytest.raises(fa.InvalidConfig):
        fa.VectorIndex.from_slab(CS.normal_rows(1, 300, 12)).build_ivf(4)            # dim % 8 != 0
    for kw in (dict(nlist=0), dict(nlist=65537), dict(nlist=int(live.sum()) + 1), dict(nlist=16, iters=65), dict(nlist=101, n_train=100)):
        with pytest.raises(fa.InvalidConfig):
            idx.build_ivf(**kw)
    bad_init = np.zeros((16, 64), dtype=F32)
    bad_init[3, 5] = np.inf
    with pytest.raises(fa.InvalidConfig):
        idx.build_ivf(16, init_centroids=bad_init)
    L = fa._lib.lib()
    from frankensearch_amd.ivf import _IvfConfig
    for field in ("reserved0", "reserved"):
        cfg = _IvfConfig()
        assert L.fsgpu_ivf_config_default(C.addressof(cfg)) == 0 and (cfg.iters, cfg.n_train) == (8, 0)
        if field == "reserved":
            cfg.reserved[2] = 1
        else:
            cfg.reserved0 = 1
        h = C.c_void_p(5)
        assert L.fsgpu_ivf_create(idx._h, 16, None, C.addressof(cfg), C.byref(h)) == fa._lib.ERR_INVALID_CONFIG and not h.value

    ivf = idx.build_ivf(300, iters=0)
    nq = 9
    q = np.ascontiguousarray(R.widen(slab[:nq]))
    rows = np.full((nq, 300), 0xABCDABCD, dtype=np.uint32)
    sc = np.full((nq, 300), 7.0, dtype=F32)
    counts = np.full(nq, 77, dtype=np.uint32)
    flags = np.full(nq, 77, dtype=np.uint32)

    def call(qlen, k, nprobe, handle=None):
        return L.fsgpu_ivf_search_batched((handle or ivf)._h, q.ctypes.data, nq, qlen, k, nprobe, rows.ctypes.data, sc.ctypes.data,
                                          counts.ctypes.data, flags.ctypes.data, None)
    assert call(64, 10, 5) == 0
    launched = ivf.stats.launches
    rows[:], sc[:], counts[:], flags[:] = 0xABCDABCD, 7.0, 77, 77
    for k, nprobe in ((0, 5), (257, 5), (10, 0), (10, 257), (256, 65), (10, 301)):
        assert call(64, k, nprobe) == fa._lib.ERR_INVALID_CONFIG, (k, nprobe)
    assert call(64, 64, 256) == 0 and ivf.stats.nprobe == 256                       # the caps themselves are served
    rows[:], sc[:], counts[:], flags[:] = 0xABCDABCD, 7.0, 77, 77
    assert call(63, 10, 5) == fa._lib.ERR_DIMENSION_MISMATCH
    small = idx.build_ivf(4, iters=0)
    assert call(64, 2, 5, small) == fa._lib.ERR_INVALID_CONFIG                      # nprobe > nlist
    chosen, sweep, n = (C.c_byte * 16)(), (C.c_byte * 64)(), C.c_uint32(5)
    probes = np.asarray([4, 400], dtype=np.uint32)
    before = ivf.stats
    assert L.fsgpu_ivf_certify_nprobe(ivf._h, q.ctypes.data, nq, probes.ctypes.data, 2, 10, 0.9, 0.1, chosen, sweep,
                                      C.byref(n)) == fa._lib.ERR_INVALID_CONFIG
    assert n.value == 5 and ivf.stats == before and launched >= 2                    # refused before any launch
    assert L.fsgpu_ivf_certify_nprobe(ivf._h, q.ctypes.data, nq, probes.ctypes.data, 0, 10, 0.9, 0.1, chosen, sweep,
                                      C.byref(n)) == fa._lib.ERR_INVALID_CONFIG
    # the hreduce order has changed: refused until it is back
    idx.set_hreduce(1)
    assert call(64, 10, 5) == fa._lib.ERR_INVALID_CONFIG and "hreduce" in fa._lib.last_error()
    with pytest.raises(fa.InvalidConfig):
        ivf.centroids()
    idx.set_hreduce(0)
    assert call(64, 10, 5) == 0
    rows[:], sc[:], counts[:], flags[:] = 0xABCDABCD, 7.0, 77, 77
    # a vacuum that removes rows: the handle is stale
    assert idx.vacuum().tombstones_removed == int((~live).sum())
    assert call(64, 10, 5) == fa._lib.ERR_INVALID_CONFIG and "stale" in fa._lib.last_error()
    assert (rows == 0xABCDABCD).all() and (sc == 7.0).all() and (counts == 77).all() and (flags == 77).all()
    for refused in (lambda: ivf.certify_nprobe(q, [4], 10, 0.9, 0.1), ivf.lists, ivf.centroids):
        with pytest.raises(fa.InvalidConfig):
            refused()
    # ... and so is a handle after compact()
    path = str(tmp_path / "ivf.fsvi")
    vec = R.widen(slab[:200])
    fa.write_fsvi(path, [(f"doc-{i:04d}", vec[i]) for i in range(200)])
    fidx = fa.VectorIndex.open(path)
    fivf = fidx.build_ivf(4, iters=1)
    r0, _, _ = fivf.search(vec[0], 5, 2)
    assert r0.size == 5
    fidx.append("doc-new", vec[1])
    assert fidx.compact().wal_records == 1
    with pytest.raises(fa.InvalidConfig):
        fivf.search(vec[0], 5, 2)


# ---- 5. the certificate ----

def test_certify_nprobe_is_the_reference_certificate(oracle):
    fa = _fa()
    c = CS.CERT
    slab, queries = CS.clustered(oracle)
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"])
    want = R.build(oracle, slab, c["nlist"], c["iters"])
    assert_build_is_reference(ivf, want, "clustered fixture")
    k = c["k"]
    er, _, ec, _ = idx.search_batched(queries, k)
    exact = [er[i, :ec[i]] for i in range(len(queries))]

    # (1) the sweep and the choice equal the restated certificate over the device's own answers
    def device_answer(p):
        rows, _, counts, flags = ivf.search_batched(queries, k, p)
        return [(rows[i, :counts[i]], flags[i]) for i in range(len(queries))]
    want_chosen, want_sweep = R.certify_nprobe(c["candidates"], device_answer, exact, c["target"], c["alpha"])
    chosen, sweep = ivf.certify_nprobe(queries, [32, 1, 8, 2, 4, 16, 4], k, c["target"], c["alpha"])
    st = ivf.stats
    print(f"chosen {chosen}, sweep {[(s.ef_search, s.certified_recall) for s in sweep]}, launches {st.launches}, rows scored {st.rows_scored}")
    assert (chosen.ef_search, chosen.certified_recall, chosen.meets_target) == want_chosen
    assert [(s.ef_search, s.certified_recall, s.meets_target) for s in sweep] == want_sweep
    # (2) nothing was launched past the choice: a coarse search and a gather scan per candidate swept
    assert chosen.meets_target and st.nprobe == chosen.ef_search == sweep[-1].ef_search
    assert st.launches == 2 * len(sweep) and st.queries == len(queries) * len(sweep)
    # (3) the choice equals ivf_ref's
    exact_ref = CS.exact_rows(oracle, slab, queries, k)
    ref_chosen, ref_sweep = R.certify_nprobe(c["candidates"], lambda p: [R.search(oracle, slab, want, q, k, p)[::2] for q in queries],
                                             exact_ref, c["target"], c["alpha"])
    assert want_chosen == ref_chosen and want_sweep == ref_sweep and ref_chosen[0] <= 16
    # an unreachable target sweeps every candidate and reports the best bound
    chosen, sweep = ivf.certify_nprobe(queries, [1, 2], k, 1.5, c["alpha"])
    assert not chosen.meets_target and [s.ef_search for s in sweep] == [1, 2] and chosen.certified_recall == max(s.certified_recall for s in sweep)

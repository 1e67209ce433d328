"""GPU checks of the IVF index (fsgpu_ivf_*) at the shapes tests/test_gpu_ivf.py leaves out — the assignment's other compile-time
dimensions and its 128- and 64-thread forms, a second assignment launch, workgroups without a gated row; in the search plan lists
of one tile, probed empty lists, ragged chunks of centroids in both coarse forms, the coarse step above 32,768 centroids, a block
walking several tiles, wide rows, non-finite queries.  Every comparison is bit for bit against tests/ivf_ref.py: centroid f32
bits, offsets and rows of a build; rows, score bits, counts, flags and the counters of a search.  tests/test_ivf_contract.py
shows without a GPU that each fixture reaches the branch it aims at."""
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
from test_gpu_ivf import _fa, assert_build_is_reference  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = R.bits
LADDER = CS.wave_ladder()


def _oracle():
    from oracle import oracle
    oracle.build()
    return oracle


# ---- A. build == ivf_ref.build ----

@pytest.mark.parametrize("dim,hreduces", [(128, (0, 1, 2)), (256, (0, 1, 2)), (384, (1, 2))])
def test_build_is_the_reference_at_the_fixed_dimensions(oracle, dim, hreduces):
    fa = _fa()
    assert CS.join_tile_plan(dim)[4]   # the compile-time form
    slab = CS.normal_rows(dim, 1000, dim)
    idx = fa.VectorIndex.from_slab(slab)
    for hreduce in hreduces:
        idx.set_hreduce(hreduce)
        ivf = idx.build_ivf(19, iters=2)
        assert_build_is_reference(ivf, R.build(oracle, slab, 19, 2, hreduce=hreduce), f"dim {dim} hreduce {hreduce}")


@pytest.mark.parametrize("step,waves,hreduce", [("last4", 4, 0), ("first2", 2, 1), ("first1", 1, 2), (1000, 1, 0), ("largest", 1, 1)])
def test_build_is_the_reference_down_the_wave_ladder(oracle, step, waves, hreduce):
    """The assignment's workgroup has 256, 128 or 64 threads by what fits the LDS (plan_join_tile, restated in ivf_cases.py)."""
    fa = _fa()
    dim = LADDER.get(step, step)
    assert CS.join_tile_plan(dim)[0] == waves and CS.build_supported(dim)
    slab = CS.normal_rows(dim, 600, dim)
    idx = fa.VectorIndex.from_slab(slab)
    idx.set_hreduce(hreduce)
    ivf = idx.build_ivf(19, iters=1)
    assert_build_is_reference(ivf, R.build(oracle, slab, 19, 1, hreduce=hreduce), f"dim {dim}, {waves} waves, hreduce {hreduce}")


def test_the_first_dimension_that_does_not_fit_is_refused():
    """The gather scan's tile gives out before the assignment's (ivf_cases.wave_ladder): the build refuses by the smaller of the two."""
    fa = _fa()
    dim = LADDER["refused"]
    assert CS.build_supported(dim - 8) and not CS.build_supported(dim)
    idx = fa.VectorIndex.from_slab(CS.normal_rows(dim, 600, dim))
    with pytest.raises(fa.InvalidConfig):
        idx.build_ivf(19, iters=1)
    assert fa.VectorIndex.from_slab(CS.normal_rows(dim - 8, 100, dim - 8)).build_ivf(3, iters=0).nlist() == 3


@pytest.mark.parametrize("n_train", [0, 5000])
def test_build_is_the_reference_over_two_assignment_launches(oracle, n_train):
    """2^20 + 300 rows: the second launch has row0 = 2^20; a dead run of 200 rows lies across the boundary."""
    fa = _fa()
    slab, live, nlist = CS.two_launch_corpus()
    assert slab.shape[0] > CS.IVF_LAUNCH_ROWS
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(nlist, iters=1, n_train=n_train)
    want = R.build(oracle, slab, nlist, 1, n_train=n_train, live=live)
    assert_build_is_reference(ivf, want, f"two launches, n_train {n_train}")
    _, rows = ivf.lists()
    assert int((rows >= CS.IVF_LAUNCH_ROWS).sum()) == int(live[CS.IVF_LAUNCH_ROWS:].sum())
    st = ivf.build_stats
    print(f"{slab.shape[0]} x 8, nlist 3, iters 1, n_train {n_train}: assign {st.assign_ms:.3f} ms, update {st.update_ms:.3f} ms, lists {st.lists_ms:.3f} ms")


@pytest.mark.parametrize("dead,n_train", [("tiles", 0), ("tiles", 40), ("sevenths", 40)])
def test_workgroups_without_a_gated_row_leave_their_rows_out(oracle, dead, n_train):
    """Eight whole 64-row workgroups dead, and a training sample of 40 rows: a workgroup without a gated row returns before it
    loads anything, and the 0xff prefill of its rows is what the lists are made from."""
    fa = _fa()
    c = CS.DEAD_TILES
    slab = CS.hashmix(oracle)
    live = CS.dead_tiles_live() if dead == "tiles" else CS.one_in_seven_dead(4099)
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"], n_train=n_train)
    want = R.build(oracle, slab, c["nlist"], c["iters"], n_train=n_train, live=live)
    assert_build_is_reference(ivf, want, f"dead {dead}, n_train {n_train}")   # lists, offsets, rows_changed_last
    _, rows = ivf.lists()
    assert rows.size == int(live.sum()) and live[rows].all()


@pytest.mark.parametrize("iters", [0, 2])
def test_a_callers_first_and_last_list_stay_empty(oracle, iters):
    fa = _fa()
    slab = CS.hashmix(oracle)
    live = CS.one_in_seven_dead(4099)
    init = CS.empty_ends_init(slab)
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(5, iters=iters, init_centroids=init)
    assert_build_is_reference(ivf, R.build(oracle, slab, 5, iters, live=live, init=init), f"empty ends, iters {iters}")
    offsets, _ = ivf.lists()
    assert offsets[0] == offsets[1] == 0 and offsets[-2] == offsets[-1] == int(live.sum())
    assert ivf.build_stats.empty_lists == 2 and (bits(ivf.centroids()[[0, -1]]) == bits(init[[0, -1]])).all()


# ---- B. search == ivf_ref.search ----

class Case:
    """An index on the device, its reference, queries and their exact score table; the reference's answers are kept per (k, nprobe)
    and query, since they do not depend on the batch."""

    def __init__(self, fa, idx, ivf, slab, want, queries, live=None):
        self.fa, self.idx, self.ivf, self.slab, self.want, self.queries, self.live = fa, idx, ivf, slab, want, queries, live
        self.oracle = _oracle()
        self.table = CS.score_table(self.oracle, slab, queries, want.hreduce)
        self.memo = {}

    def reference(self, i, k, nprobe):
        key = (i, k, nprobe)
        if key not in self.memo:
            self.memo[key] = R.search(self.oracle, self.slab, self.want, self.queries[i], k, nprobe, row_scores=self.table[i],
                                      exact=CS.exact_from_scores(self.table[i])) + (R.rows_scored(self.oracle, self.want, self.queries[i], nprobe),)
        return self.memo[key]

    def answer(self, pick, k, nprobe, form):
        q = np.ascontiguousarray(self.queries[pick])
        nq = q.shape[0]
        if form == "host":
            return self.ivf.search_batched(q, k, nprobe)
        import torch
        dq = torch.from_numpy(q).cuda()
        drows = torch.full((nq, k), 7, dtype=torch.int32, device="cuda")
        dsc = torch.zeros((nq, k), dtype=torch.float32, device="cuda")
        dcounts = torch.full((nq,), 77, dtype=torch.int32, device="cuda")
        dflags = torch.full((nq,), 9, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        self.ivf.search_batched_device(dq.data_ptr(), nq, k, nprobe, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
        return (drows.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dcounts.cpu().numpy().view(np.uint32),
                dflags.cpu().numpy().view(np.uint32))

    def check(self, k, nprobe, nq=None, form="host", pick=None):
        """-> the number of queries per flag."""
        pick = np.arange(len(self.queries) if nq is None else nq) if pick is None else np.asarray(pick)
        rows, sc, counts, flags = self.answer(pick, k, nprobe, form)
        st = self.ivf.stats
        bad, flagged, scored = [], [0, 0, 0], 0
        for pos, i in enumerate(pick):
            wr, ws, wf, wn = self.reference(int(i), k, nprobe)
            flagged[wf] += 1
            scored += wn
            if not (counts[pos] == wr.size and flags[pos] == wf and (rows[pos, :wr.size] == wr).all() and (bits(sc[pos, :wr.size]) == bits(ws)).all()):
                bad.append(int(i))
        what = f"k {k} nprobe {nprobe} nq {len(pick)} {form}"
        assert not bad, f"{what}: queries {bad[:8]} differ ({len(bad)} of {len(pick)})"
        assert (st.approximate, st.underfilled, st.empty_despite_indexed_points) == tuple(flagged), what
        assert (st.queries, st.nprobe, st.k_requested, st.nlist, st.lists_probed, st.rows_scored) == \
            (len(pick), nprobe, k, self.want.offsets.size - 1, len(pick) * nprobe, scored), what
        return flagged


def _built(slab, nlist, iters, queries, live=None, hreduce=0, check_build=True):
    fa, oracle = _fa(), _oracle()
    idx = fa.VectorIndex.from_slab(slab, live=live)
    idx.set_hreduce(hreduce)   # before the build: the handle records the order
    ivf = idx.build_ivf(nlist, iters=iters)
    if check_build:
        want = R.build(oracle, slab, nlist, iters, live=live, hreduce=hreduce)
        assert_build_is_reference(ivf, want, f"nlist {nlist} iters {iters} hreduce {hreduce}")
    else:   # the device's own index: the search alone is under test
        offsets, rows = ivf.lists()
        st = ivf.build_stats
        want = R.Index(ivf.centroids(), offsets, rows, np.ones(slab.shape[0], dtype=bool) if live is None else live.copy(), hreduce,
                       st.rows_trained, st.rows_changed_last)
    return Case(fa, idx, ivf, slab, want, queries, live)


# -- 1. one tile per probed list --

@functools.lru_cache(maxsize=None)
def one_tile_case(which):
    c = CS.ONE_TILE
    slab, live = CS.one_tile_corpus(_oracle(), which)
    return _built(slab, c["nlist"], c["iters"], CS.noisy_queries(slab, c["nq"], 64), live=live)


@pytest.mark.parametrize("which", ["normal", "hashmix"])
def test_search_is_the_reference_where_a_probed_list_is_one_tile(oracle, which):
    """"normal": every list has at most 64 rows, so every probed list has one scan block and the per-query merge reads the scan's
    table, whose rows are 64 entries apart for k <= 64; many lists are shorter than k, and the underfilled queries' answers are the
    exact search's.  "hashmix": lists of two tiles among empty ones by the hundred (ivf_cases.one_tile_corpus)."""
    c = CS.ONE_TILE
    case = one_tile_case(which)
    lens = np.diff(case.want.offsets.astype(np.int64))
    assert (lens.max() <= CS.GATHER_TILE_ROWS) == (which == "normal")
    served = [(k, p) for k in c["ks"] for p in c["nprobes"] if CS.call_ok(64, c["nlist"], k, p)]
    assert len(served) == 23
    total = [0, 0, 0]
    for k, nprobe in served:
        flagged = case.check(k, nprobe)
        total = [a + b for a, b in zip(total, flagged)]
    case.check(10, 5, form="device")
    case.check(64, 1, form="device")   # the fallback through the device form
    print(f"{which}: approximate / underfilled / empty {total}")
    assert total[0] > 0 and total[1] + total[2] > 0
    # the fallback's answers are the handle's exact search
    k = 64
    rows, sc, counts, flags = case.ivf.search_batched(case.queries, k, 1)
    er, es, ec = case.idx.search_batch(case.queries, k, exact=True)
    under = np.nonzero(flags)[0]
    assert under.size > 0
    for i in under:
        assert counts[i] == ec[i] and (rows[i, :ec[i]] == er[i, :ec[i]]).all() and (bits(sc[i, :ec[i]]) == bits(es[i, :ec[i]])).all()


# -- 2. empty probed lists --

@functools.lru_cache(maxsize=None)
def duplicate_case(iters):
    slab, nlist = CS.duplicate_corpus()
    return _built(slab, nlist, iters, CS.duplicate_queries())


@pytest.mark.parametrize("iters", [0, 1])
def test_a_probed_empty_list_owns_no_slot_and_is_counted(oracle, iters):
    """nprobe 2 probes a query's twin lists, one of which is empty; nprobe 4 has lists with members AFTER an empty one."""
    case = duplicate_case(iters)
    nq = len(case.queries)
    for nprobe in (1, 2, 4, 128):
        for k in (10, 50, 64, 100):
            case.check(k, nprobe)
            st = case.ivf.stats
            assert st.lists_probed == nq * nprobe                       # the empty lists are counted ...
            if iters == 0:   # ... and add no rows: twins score alike to the bit, so every other probed list is the empty one
                assert st.rows_scored == 50 * nq * ((nprobe + 1) // 2)
    case.check(10, 2, form="device")
    case.check(64, 4, form="device")


# -- 3. ragged chunks of centroids --

@functools.lru_cache(maxsize=None)
def ragged_case(dim, nlist, hreduce):
    c = CS.RAGGED
    slab = CS.normal_rows(1000 + dim + nlist, c["n"], dim)
    return _built(slab, nlist, c["iters"], CS.noisy_queries(slab, max(c["nqs"]), dim + nlist), hreduce=hreduce)


@pytest.mark.parametrize("dim,nlist,hreduce", CS.ragged_cases())
def test_a_ragged_last_chunk_of_centroids_in_both_coarse_forms(oracle, dim, nlist, hreduce):
    c = CS.RAGGED
    case = ragged_case(dim, nlist, hreduce)
    forms = set()
    for nq in c["nqs"]:
        for nprobe in c["nprobes"]:
            if nprobe <= nlist:
                case.check(c["k"], nprobe, nq=nq)
                forms.add(CS.coarse_is_join(nq, nprobe, dim))
    assert forms == {True, False}
    case.check(c["k"], 17, nq=16, form="device")   # the join
    case.check(c["k"], 17, nq=15, form="device")   # the centroid index


# -- 4. the coarse step above 32,768 centroids --

@functools.lru_cache(maxsize=None)
def many_lists_case(dim):
    c = CS.MANY_LISTS
    slab = CS.many_lists_corpus(dim)
    return _built(slab, c["nlist"], c["iters"], CS.noisy_queries(slab, 40, 43), check_build=False)


@pytest.mark.parametrize("dim", CS.MANY_LISTS["dims"])
def test_the_coarse_step_over_40000_centroids(oracle, dim):
    """The centroid index is an F32 index of 40,000 rows.  At dim 64 its batched search goes through the int8 matrix-core filter
    (from 32,768 rows, k = nprobe <= 64): 40 queries at nprobe 64 build the int8 copy and use it, 8 queries at nprobe 64 and 5 then
    find it ready, 40 queries at nprobe 5 take the join.  At dim 16, which the matrix-core scan does not serve, the same calls are
    the exact F32 kernels and the join over 40,000 centroids.  ivf_cases.coarse_by_int8_filter restates the gate and
    test_ivf_contract.py pins it to the source; the ABI does not report which path answered.  The calls run in MANY_LISTS' order.
    The BUILD of this case is not under test: centroids and lists are read back from the device and the search alone is compared."""
    c = CS.MANY_LISTS
    case = many_lists_case(dim)
    ready = False
    for nq, nprobe in c["calls"]:
        filtered = CS.coarse_by_int8_filter(c["nlist"], dim, nq, nprobe, ready)
        assert filtered == (dim == 64 and not CS.coarse_is_join(nq, nprobe, dim))
        ready = ready or filtered
        case.check(c["k"], nprobe, nq=nq)
        case.check(c["k"], nprobe, nq=nq, form="device")


# -- 5. many probed groups --

@functools.lru_cache(maxsize=None)
def many_groups_case():
    slab = CS.normal_rows(47, 200000, 16)
    return _built(slab, 2048, 0, CS.noisy_queries(slab, 257, 53), check_build=False)


@pytest.mark.parametrize("k", [10, 100])
def test_many_probed_groups_with_a_block_walking_several_tiles(oracle, k):
    """257 queries x nprobe 16 over 2,048 lists, a quarter of them longer than a tile and the longest of some 60 tiles: hundreds of
    probed groups, and with so many a list gets few blocks — one, once the groups outnumber two per compute unit — which then walks
    the list's tiles in turn.  Which side of that threshold a card lands on is not asserted: the answer does not depend on it.
    The BUILD of this case is not under test: centroids and lists are read back from the device and the search alone is compared."""
    case = many_groups_case()
    lens = np.diff(case.want.offsets.astype(np.int64))
    assert (lens > CS.GATHER_TILE_ROWS).sum() > 256 and lens.max() > 16 * CS.GATHER_TILE_ROWS   # lists of several tiles
    case.check(k, 16)
    if k == 10:
        case.check(k, 16, form="device")


# -- 6. wide rows --

@functools.lru_cache(maxsize=None)
def wide_case(dim):
    c = CS.WIDE
    slab, hreduce = CS.wide_corpus(dim)
    return _built(slab, c["nlist"], c["iters"], CS.noisy_queries(slab, c["nq"], dim + 1), hreduce=hreduce)


@pytest.mark.parametrize("dim", CS.WIDE["dims"])
def test_wide_rows_are_served_up_to_the_gather_scans_cap(oracle, dim):
    case = wide_case(dim)
    for k in CS.WIDE["ks"]:
        assert CS.gather_supported(dim, k)
        for nprobe in CS.WIDE["nprobes"]:
            case.check(k, nprobe, nq=20)   # the join
            case.check(k, nprobe, nq=9)    # the centroid index
    case.check(10, 5, nq=20, form="device")
    # k = 65 asks for the scan's 256-entry buffers
    if CS.gather_supported(dim, 65):
        case.check(65, 5, nq=20)
        return
    fa, ivf = case.fa, case.ivf
    nq = 9
    q = np.ascontiguousarray(case.queries[:nq])
    rows = np.full((nq, 65), 0xABCDABCD, dtype=np.uint32)
    sc = np.full((nq, 65), 7.0, dtype=F32)
    counts = np.full(nq, 77, dtype=np.uint32)
    flags = np.full(nq, 77, dtype=np.uint32)
    before = ivf.stats
    rc = fa._lib.lib().fsgpu_ivf_search_batched(ivf._h, q.ctypes.data, nq, dim, 65, 5, rows.ctypes.data, sc.ctypes.data, counts.ctypes.data,
                                               flags.ctypes.data, None)
    assert rc == fa._lib.ERR_INVALID_CONFIG
    assert (rows == 0xABCDABCD).all() and (sc == 7.0).all() and (counts == 77).all() and (flags == 77).all() and ivf.stats == before
    with pytest.raises(fa.InvalidConfig):
        ivf.search_batched(q, 65, 5)


# -- 7. non-finite queries --

@functools.lru_cache(maxsize=None)
def nonfinite_query_case():
    c = CS.NONFINITE_Q
    slab = CS.hashmix(_oracle())
    return _built(slab, c["nlist"], c["iters"], CS.nonfinite_queries(slab, c["nq"], c["at"]), live=CS.one_in_seven_dead(4099))


def test_non_finite_queries_follow_the_order_in_both_coarse_forms(oracle):
    """A query with a NaN (every score NaN: NaN sorts as -inf, the lower id first — among centroids and among rows), one with a
    +inf, the all-zero query."""
    c = CS.NONFINITE_Q
    case = nonfinite_query_case()
    q, (nan_q, inf_q, zero_q), k, nprobe = case.queries, c["at"], c["k"], c["nprobe"]
    assert np.isnan(q[nan_q]).any() and np.isinf(q[inf_q]).any() and not q[zero_q].any()
    assert np.isnan(case.table[nan_q]).all() and not np.isfinite(case.table[inf_q]).any() and not case.table[zero_q].any()
    assert CS.coarse_is_join(c["nq"], nprobe, 64) and not CS.coarse_is_join(3, nprobe, 64)
    case.check(k, nprobe)                      # the join, the three among finite queries
    case.check(k, nprobe, pick=c["at"])        # the centroid index
    case.check(k, nprobe, form="device")
    case.check(k, nprobe, pick=c["at"], form="device")
    # the NaN query's probed lists are the five lowest centroids and its rows the ten lowest of their live rows
    wr, ws, wf, _ = case.reference(nan_q, k, nprobe)
    assert wf == R.APPROXIMATE and np.isnan(ws).all()
    assert wr.tolist() == np.sort(np.concatenate([case.want.list_rows(l) for l in range(nprobe)]))[:k].tolist()

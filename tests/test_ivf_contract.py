"""The IVF index's contract without a GPU: tests/ivf_ref.py against itself and against the oracle's exact search, the fixtures of
tests/ivf_cases.py against their own preconditions, one broken rule at a time, and the caps against kernels.hpp's constants."""
import os
import re

import numpy as np
import pytest

import ivf_cases as CS
import ivf_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
bits = R.bits


@pytest.fixture(scope="module")
def small(oracle):
    slab = CS.normal_rows(3, 1500, 24)
    queries = np.random.default_rng(4).standard_normal((12, 24)).astype(np.float32)
    return slab, queries, R.build(oracle, slab, 12, 2)


# ---- nesting ----

def test_recall_is_monotone_in_nprobe_and_every_list_probed_is_the_exact_search(oracle, small):
    slab, queries, index = small
    k = 10
    for q in queries:
        er, es = oracle.search_top_k(slab, q, k)
        last = -1.0
        for nprobe in (1, 2, 3, 6, 12):
            rows, scores, flag = R.search(oracle, slab, index, q, k, nprobe)
            assert flag == R.APPROXIMATE and rows.size == k
            rec = len(set(rows.tolist()) & set(er.tolist())) / k
            assert rec >= last   # candidate sets nest
            last = rec
        assert (rows == er).all() and (bits(scores) == bits(es)).all()   # nprobe == nlist


def test_lists_partition_the_live_rows_in_ascending_order(oracle):
    slab = CS.normal_rows(5, 700, 16)
    live = CS.one_in_seven_dead(700)
    index = R.build(oracle, slab, 9, 1, n_train=100, live=live)
    assert index.trained == int(live[R.training_rows(700, 100)].sum())
    assert sorted(index.rows.tolist()) == np.nonzero(live)[0].tolist()
    for l in range(9):
        lr = index.list_rows(l)
        assert (np.diff(lr.astype(np.int64)) > 0).all()
    norms = np.linalg.norm(index.centroids.astype(np.float64), axis=1)
    assert np.allclose(norms, 1.0, atol=1e-6)


# ---- the fixtures satisfy their own preconditions ----

def test_the_duplicate_corpus_leaves_the_higher_twin_empty(oracle):
    slab, nlist = CS.duplicate_corpus()
    init = R.strided_init(slab, R.training_rows(slab.shape[0], 0), nlist)
    assert (bits(init[0::2]) == bits(init[1::2])).all()
    lens = np.diff(R.build(oracle, slab, nlist, 0).offsets.astype(np.int64))   # the assignment alone: the lower twin takes every row
    assert (lens[1::2] == 0).all() and (lens[0::2] == 50).all()
    index = R.build(oracle, slab, nlist, 1)   # ... and so does the iteration's, which leaves the higher twin without members
    assert (bits(index.centroids[1::2]) == bits(init[1::2])).all()         # an empty list keeps its bits
    assert not (bits(index.centroids[0::2]) == bits(init[0::2])).all()     # its twin was updated


def test_the_underfill_corpus_has_a_short_probed_list(oracle):
    slab, init, query, short = CS.underfill_corpus()
    index = R.build(oracle, slab, 2, 1, init=init)
    assert R.probe(oracle, index, query, 1).tolist() == [1] and index.list_rows(1).tolist() == short.tolist()
    rows, scores, flag = R.search(oracle, slab, index, query, 10, 1)
    er, es = oracle.search_top_k(slab, query, 10)
    assert flag == R.UNDERFILLED and (rows == er).all() and (bits(scores) == bits(es)).all()
    live = np.ones(slab.shape[0], dtype=bool)
    live[short] = False
    rows, scores, flag = R.search(oracle, slab, index, query, 10, 1, live_now=live)
    er, es = oracle.search_top_k(slab, query, 10, live=live)
    assert flag == R.EMPTY and (rows == er).all() and (bits(scores) == bits(es)).all()


def test_the_nonfinite_corpus_has_lists_whose_norm_is_not_finite(oracle):
    slab, nlist = CS.nonfinite_corpus()
    wide = R.widen(slab)
    init = R.strided_init(slab, R.training_rows(slab.shape[0], 0), nlist)
    assert np.isfinite(init).all()
    a = R.assign(R.centroid_scores(oracle, slab, init), np.ones(slab.shape[0], dtype=bool))
    assert a[5] == 0 and a[17] == 0                                        # every score NaN: list 0
    bad = [l for l in range(nlist) if not np.isfinite(R.list_mean_norm2(wide, np.nonzero(a == l)[0])[1])]
    assert 0 in bad and len(bad) >= 2
    index = R.build(oracle, slab, nlist, 1)
    for l in range(nlist):
        assert (bits(index.centroids[l]) == bits(init[l])).all() == (l in bad)   # ... keeps its centroid, the others move
    assert np.isfinite(index.centroids).all()


def test_the_two_launch_corpus_crosses_the_launch_boundary_with_an_ungated_run(oracle):
    slab, live, nlist = CS.two_launch_corpus()
    n, edge = slab.shape[0], CS.IVF_LAUNCH_ROWS
    assert n > edge and (n - edge) % 64 != 0                       # a second launch, row0 = 2^20, its last tile ragged
    assert not live[edge - 150:edge + 50].any() and live[edge - 157:edge - 150].sum() == 6 and live[edge + 50:edge + 57].sum() == 6
    assert (edge - 150) // 64 + 1 < edge // 64                     # whole ungated tiles before the edge, most of one after it
    assert live[edge + 64:].sum() > 100
    for n_train in (0, 5000):
        train = R.training_rows(n, n_train, live)
        assert (train >= edge).any() and (train < edge).any() and len(train) >= nlist
    index = R.build(oracle, slab, nlist, 1, live=live)
    past = [int((index.list_rows(l) >= edge).sum()) for l in range(nlist)]
    assert min(past) > 0 and sum(past) == int(live[edge:].sum())   # every list has members from the second launch


def test_the_dead_tiles_leave_whole_workgroups_ungated(oracle):
    c = CS.DEAD_TILES
    live = CS.dead_tiles_live()
    assert CS.join_tile_plan(64)[0] * CS.JOIN_ROWS_PER_WAVE == 64   # rows per workgroup at dim 64
    tiles = lambda gate: np.add.reduceat(gate.astype(np.int64), np.arange(0, gate.size, 64))
    assert (tiles(live)[4:12] == 0).all() and (tiles(live)[:4] == 64).all()
    for lv in (live, CS.one_in_seven_dead(4099)):
        train = R.training_rows(4099, c["n_train"], lv)
        gate = np.zeros(4099, dtype=bool)
        gate[train] = True
        assert c["nlist"] <= len(train) <= c["n_train"] and (tiles(gate) == 0).sum() > 20   # most of the 65 tiles
    slab = CS.hashmix(oracle)
    index = R.build(oracle, slab, c["nlist"], c["iters"], n_train=c["n_train"], live=live)
    assert not np.isin(np.arange(256, 768), index.rows).any() and index.rows.size == int(live.sum())
    assert 0 < index.changed_last <= index.trained


def test_the_empty_ends_init_leaves_the_first_and_the_last_list_empty(oracle):
    slab = CS.hashmix(oracle)
    live = CS.one_in_seven_dead(4099)
    init = CS.empty_ends_init(slab)
    for iters in (0, 2):
        index = R.build(oracle, slab, 5, iters, live=live, init=init)
        lens = np.diff(index.offsets.astype(np.int64))
        assert lens[0] == 0 and lens[-1] == 0 and (lens[1:-1] > 0).all(), lens
        assert index.offsets[0] == index.offsets[1] == 0 and index.offsets[-2] == index.offsets[-1] == int(live.sum())
        assert (bits(index.centroids[[0, -1]]) == bits(init[[0, -1]])).all()


def test_the_one_tile_index_has_lists_of_one_tile_and_some_shorter_than_k(oracle):
    c = CS.ONE_TILE
    slab, live = CS.one_tile_corpus(oracle, "hashmix")   # not what its name says: two-tile lists among 255 empty ones
    lens = np.diff(R.build(oracle, slab, c["nlist"], c["iters"], live=live).offsets.astype(np.int64))
    assert (lens == 0).sum() > 200 and CS.GATHER_TILE_ROWS < lens.max() <= 2 * CS.GATHER_TILE_ROWS, (lens.max(), (lens == 0).sum())
    slab, live = CS.one_tile_corpus(oracle, "normal")
    index = R.build(oracle, slab, c["nlist"], c["iters"], live=live)
    lens = np.diff(index.offsets.astype(np.int64))
    assert 1 <= lens.min() and lens.max() <= CS.GATHER_TILE_ROWS and (lens < 10).sum() > 50, (lens.max(), lens.min())
    served = [(k, p) for k in c["ks"] for p in c["nprobes"] if CS.call_ok(64, c["nlist"], k, p)]
    assert len(served) == 23 and (256, 64) in served and (256, 256) not in served and (65, 256) not in served
    # a single probed list is shorter than 64 rows: at k = 64 and nprobe = 1 every query falls back
    queries = CS.noisy_queries(slab, c["nq"], 64)
    flags = [R.search(oracle, slab, index, q, 64, 1)[2] for q in queries]
    assert R.UNDERFILLED in flags


def test_at_nprobe_two_every_duplicate_query_probes_an_empty_list(oracle):
    slab, nlist = CS.duplicate_corpus()
    queries = CS.duplicate_queries()
    for iters in (0, 1):
        index = R.build(oracle, slab, nlist, iters)
        for c, q in enumerate(queries):
            lists = R.probe(oracle, index, q, 2).tolist()
            assert sorted(lists) == [2 * c, 2 * c + 1], (iters, c, lists)
            # (after an iteration the updated twin is normalised and the other is not: either may take the 50 rows)
            assert sorted([index.list_rows(2 * c).size, index.list_rows(2 * c + 1).size]) == [0, 50]
            assert R.rows_scored(oracle, index, q, 2) == 50
        first_is_empty = sum(index.list_rows(int(R.probe(oracle, index, q, 2)[0])).size == 0 for q in queries)
        assert first_is_empty == 0   # whichever twin scores a row higher scores the query higher: the empty one comes second


def test_the_ragged_cases_end_in_a_partial_chunk_and_reach_both_coarse_forms():
    c = CS.RAGGED
    cases = CS.ragged_cases()
    assert len(cases) == 12 and {h for _, _, h in cases} == {0, 1, 2}
    for dim in (64, 128, 256, 72):
        assert {h for d, _, h in cases if d == dim} == {0, 1, 2}   # every order at every dimension
    assert all(nlist % CS.JOIN_CHUNK != 0 for _, nlist, _ in cases)
    forms = {CS.coarse_is_join(nq, p, 64) for nq in c["nqs"] for p in c["nprobes"]}
    assert forms == {True, False}
    assert not CS.coarse_is_join(15, 1, 64) and CS.coarse_is_join(16, 63, 64) and not CS.coarse_is_join(16, 64, 64)
    assert CS.coarse_is_join(16, 5, 1000) and CS.coarse_is_join(16, 5, 520)   # the wide rows reach the join too


def test_the_many_lists_calls_reach_the_int8_filter_at_dim_64_and_only_there():
    src = os.path.join(ROOT, "frankensearch_amd", "csrc")
    batched = open(os.path.join(src, "vector_index_batched.cpp")).read()
    assert "scan_mfma_supported((int)dim_) && k >= 1 && k <= 64 && nrows_ >= 4 * 8192ull;" in batched
    assert "nq < 16 && !filter_ready() && !int8_latency) i8f = false;" in batched
    assert "(!f32_ || (p.i8f && !p.strided))" in batched   # an F32 slab without the filter: the exact kernels
    assert "bool scan_mfma_supported(int dim) { return dim == 64 || dim == 128 || dim == 256 || dim == 384; }" in \
        open(os.path.join(src, "mfma_scan.hip")).read()
    assert (CS.MFMA_DIMS, CS.I8F_MIN_ROWS, CS.I8F_MAX_K, CS.I8F_BUILD_MIN_QUERIES) == ((64, 128, 256, 384), 32768, 64, 16)
    c = CS.MANY_LISTS
    assert c["nlist"] >= CS.I8F_MIN_ROWS and c["nlist"] <= c["n"] and c["dims"] == (64, 16)
    for dim, want in ((64, ["filter", "filter", "filter", "join"]), (16, ["exact", "exact", "exact", "join"])):
        ready, forms = False, []
        for nq, nprobe in c["calls"]:
            if CS.coarse_is_join(nq, nprobe, dim):
                forms.append("join")
            elif CS.coarse_by_int8_filter(c["nlist"], dim, nq, nprobe, ready):
                forms.append("filter")
                ready = True
            else:
                forms.append("exact")
        assert forms == want, (dim, forms)
    # the small calls alone would not build the copy; the searched indexes of the other tests are all below the row count
    assert not CS.coarse_by_int8_filter(c["nlist"], 64, 8, 64, False) and not CS.coarse_by_int8_filter(c["nlist"], 64, 40, 65, True)
    assert not CS.coarse_by_int8_filter(300, 64, 40, 64, True) and not CS.coarse_by_int8_filter(2048, 16, 257, 64, True)


def test_the_wide_rows_reach_both_coarse_forms_and_fill_k(oracle):
    c = CS.WIDE
    for dim in c["dims"]:
        slab, hreduce = CS.wide_corpus(dim)
        assert dim not in CS.ASSIGN_FIXED_DIMS and dim % 32 != 0 and CS.build_supported(dim) and dim <= CS.KNN_UPD_MAX_DIM
        assert CS.join_tile_plan(dim)[0] == (2 if dim == 520 else 1)
        assert all(CS.call_ok(dim, c["nlist"], k, p) for k in c["ks"] for p in c["nprobes"])
        assert CS.call_ok(dim, c["nlist"], 65, 5) == (dim == 520)
        assert {CS.coarse_is_join(nq, p, dim) for nq in (c["nq"], 9) for p in c["nprobes"]} == {True, False}
        index = R.build(oracle, slab, c["nlist"], c["iters"], hreduce=hreduce)
        lens = np.diff(index.offsets.astype(np.int64))
        assert lens.min() >= max(c["ks"]) and lens.max() > CS.GATHER_TILE_ROWS   # every list fills k, some take several tiles
        q = CS.noisy_queries(slab, c["nq"], dim + 1)[0]
        rows, scores, flag = R.search(oracle, slab, index, q, 64, c["nlist"])
        er, es = oracle.search_top_k(slab, q, 64, hreduce=hreduce)
        assert flag == R.APPROXIMATE and (rows == er).all() and (bits(scores) == bits(es)).all()   # every list probed: the exact search


def test_the_non_finite_queries_score_as_their_docstring_says(oracle):
    c = CS.NONFINITE_Q
    slab = CS.hashmix(oracle)
    live = CS.one_in_seven_dead(4099)
    q = CS.nonfinite_queries(slab, c["nq"], c["at"])
    nan_q, inf_q, zero_q = c["at"]
    assert np.isnan(q[nan_q]).sum() == 1 and np.isinf(q[inf_q]).sum() == 1 and not q[zero_q].any()
    assert np.isfinite(np.delete(q, c["at"], axis=0)).all()
    assert CS.coarse_is_join(c["nq"], c["nprobe"], 64) and not CS.coarse_is_join(len(c["at"]), c["nprobe"], 64)
    table = CS.score_table(oracle, slab, q[list(c["at"])])
    assert np.isnan(table[0]).all() and not table[2].any()
    assert np.isposinf(table[1]).any() and np.isneginf(table[1]).any() and not np.isfinite(table[1]).any()
    index = R.build(oracle, slab, c["nlist"], c["iters"], live=live)
    lowest = np.sort(np.concatenate([index.list_rows(l) for l in range(c["nprobe"])]))[:c["k"]]
    for i, qi in ((0, nan_q), (2, zero_q)):   # every centroid and every row ties: the lower id first, among both
        assert R.probe(oracle, index, q[qi], c["nprobe"]).tolist() == list(range(c["nprobe"]))
        rows, scores, flag = R.search(oracle, slab, index, q[qi], c["k"], c["nprobe"], row_scores=table[i])
        assert flag == R.APPROXIMATE and rows.tolist() == lowest.tolist()
    lists = R.probe(oracle, index, q[inf_q], c["nprobe"])
    assert lists.tolist() != list(range(c["nprobe"]))   # the +inf query does order the centroids
    rows, scores, flag = R.search(oracle, slab, index, q[inf_q], c["k"], c["nprobe"], row_scores=table[1])
    assert flag == R.APPROXIMATE and np.isposinf(scores).all() and (np.diff(rows.astype(np.int64)) > 0).all()


def test_the_wave_ladder_is_join_tile_hpp_restated():
    kern = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "kernels.hpp")).read()
    tile = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "join_tile.hpp")).read()
    ivf = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "ivf_kernels.hip")).read()
    host = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "ivf_index.cpp")).read()

    def const(name):
        m = re.search(r"\b" + name + r"\s*=\s*([0-9 *<u]+)[;,]", kern)
        assert m, name
        return int(eval(m.group(1).replace("u", "").replace("<<", " << ")))
    assert (const("kJoinTileRowsPerWave"), const("kJoinTileChunk")) == (CS.JOIN_ROWS_PER_WAVE, CS.JOIN_CHUNK)
    assert const("kIvfLdsBudget") == CS.IVF_LDS_BUDGET and const("kIvfLaunchRows") == CS.IVF_LAUNCH_ROWS == R.LAUNCH_ROWS
    assert (const("kKnnMaxM"), const("kKnnUpdMaxDim")) == (CS.KNN_MAX_M, CS.KNN_UPD_MAX_DIM)
    assert const("kGatherTileRows") == R.TILE_ROWS
    assert "JoinTilePlan p{4, (int)((dim + 15u) & ~15u) + 8, (int)((dim + 1u) & ~1u), 0, false};" in tile
    assert "((size_t)waves * kJoinTileRowsPerWave * p.xstride + (size_t)kJoinTileChunk * p.qstride) * 4 + waves * extra_per_wave" in tile
    assert ivf.count("plan_join_tile(a.dim, 0, kIvfLdsBudget, {384, 256, 128, 64})") == 1 and CS.ASSIGN_FIXED_DIMS == (384, 256, 128, 64)
    assert "nq >= 16 && nprobe <= kKnnMaxM && dim <= kKnnUpdMaxDim" in host
    assert "!filter_gather_supported(dim, 1) || !ivf_assign_supported(dim)" in host
    # the plan at the dimensions the tests use
    assert CS.join_tile_plan(64) == (4, 72, 64, (64 * 72 + 16 * 64) * 4, True)
    assert CS.join_tile_plan(72) == (4, 88, 72, (64 * 88 + 16 * 72) * 4, False)
    for dim in CS.ASSIGN_FIXED_DIMS:
        assert CS.join_tile_plan(dim)[4]
    lad = CS.wave_ladder()
    assert (lad["last4"], lad["first2"]) == (496, 504) and lad["first2"] == lad["last4"] + 8
    waves = lambda d: CS.join_tile_plan(d)[0]
    assert waves(lad["first1"] - 8) == 2 and waves(lad["first1"]) == 1 and waves(1000) == 1 and lad["first1"] < 1000
    for d in (lad["last4"], lad["first2"], lad["first1"], 1000, lad["largest"]):
        assert 0 < CS.join_tile_plan(d)[3] <= CS.IVF_LDS_BUDGET and CS.build_supported(d) and not CS.join_tile_plan(d)[4]
    # the assignment's own refusal lies behind the gather scan's: a build is refused by the smaller of the two
    top_assign = max(d for d in range(8, 4096, 8) if CS.assign_supported(d))
    assert not CS.assign_supported(top_assign + 8) and CS.join_tile_plan(top_assign + 8)[3] == 0
    assert lad["largest"] < top_assign and lad["refused"] == lad["largest"] + 8
    assert CS.assign_supported(lad["refused"]) and not CS.gather_supported(lad["refused"], 1)
    assert waves(lad["largest"]) == 1
    # the wide rows of the search tests: served at k <= 64; k = 65 asks for the 256-entry buffers, which 1000 does not fit
    assert CS.gather_supported(520, 64) and CS.gather_supported(1000, 64) and CS.gather_supported(520, 65) and not CS.gather_supported(1000, 65)


# ---- the certificate on the clustered fixture ----

def test_the_restated_certificate_chooses_a_small_nprobe_on_the_clustered_fixture(oracle):
    c = CS.CERT
    slab, queries = CS.clustered(oracle)
    index = R.build(oracle, slab, c["nlist"], c["iters"])
    exact = CS.exact_rows(oracle, slab, queries, c["k"])
    launched = []

    def answer(p):
        launched.append(p)
        return [R.search(oracle, slab, index, q, c["k"], p)[::2] for q in queries]
    chosen, sweep = R.certify_nprobe(c["candidates"], answer, exact, c["target"], c["alpha"])
    print("sweep", sweep)
    assert chosen[2] and chosen[0] <= 16 and chosen[1] >= c["target"]
    assert launched == [s[0] for s in sweep] and launched[-1] == chosen[0]   # nothing past the choice
    assert [s[1] for s in sweep] == sorted(s[1] for s in sweep)              # bounds nest with the candidate sets


# ---- one rule broken at a time ----

def _differs(a, b):
    return not (a.shape == b.shape and (bits(a) == bits(b)).all())


def test_every_rule_is_reached_by_the_case_aimed_at_it(oracle):
    # ties to the higher centroid: the duplicate corpus fills the other twin
    slab, nlist = CS.duplicate_corpus()
    good, bad = R.build(oracle, slab, nlist, 0), R.build(oracle, slab, nlist, 0, rules={"ties_high"})
    assert (good.offsets != bad.offsets).any()
    # a pairwise sum: centroid bits differ where the sum depends on its order (sums of f16 values are exact in f64 until they span
    # more than 53 bits: random rows do not reach the rule, the cancelling corpus does)
    slab, one = CS.cancelling_corpus()
    good = R.build(oracle, slab, one, 1)
    assert np.isfinite(good.centroids).all() and abs(np.linalg.norm(good.centroids[0].astype(np.float64)) - 1.0) < 1e-6
    assert _differs(good.centroids, R.build(oracle, slab, one, 1, rules={"pairwise_sum"}).centroids)
    # no normalisation
    slab = CS.normal_rows(3, 1500, 24)
    good = R.build(oracle, slab, 12, 1)
    assert _differs(good.centroids, R.build(oracle, slab, 12, 1, rules={"no_normalise"}).centroids)
    # an empty list re-seeded
    slab, nlist = CS.duplicate_corpus()
    assert _differs(R.build(oracle, slab, nlist, 1).centroids, R.build(oracle, slab, nlist, 1, rules={"reseed_empty"}).centroids)
    # the dead-row test made at build time only
    slab, init, query, short = CS.underfill_corpus()
    index = R.build(oracle, slab, 2, 1, init=init)
    live = np.ones(slab.shape[0], dtype=bool)
    live[short[0]] = False
    rows, _, flag = R.search(oracle, slab, index, query, 2, 1, live_now=live)
    rows_bad, _, flag_bad = R.search(oracle, slab, index, query, 3, 1, live_now=live, rules={"dead_at_build"})
    assert flag == flag_bad == R.APPROXIMATE and short[0] in rows_bad and sorted(rows.tolist()) == short[1:].tolist()
    # one-tile lists read k apart instead of 64 apart: the second probed list's entries come from the first's padding
    c = CS.ONE_TILE
    slab, live = CS.one_tile_corpus(oracle, "normal")
    index = R.build(oracle, slab, c["nlist"], c["iters"], live=live)
    queries = CS.noisy_queries(slab, c["nq"], 64)
    for k, nprobe, least in ((10, 5, 17), (1, 5, 1), (10, 63, 17)):   # (k = 1: only a query whose best row is not in its first list)
        changed = 0
        for q in queries:
            good, bad = R.search(oracle, slab, index, q, k, nprobe), R.search(oracle, slab, index, q, k, nprobe, rules={"stride_k_tiles"})
            changed += good[2] != bad[2] or _differs(good[0], bad[0])
        assert changed >= least, (k, nprobe, changed)
    q = queries[0]
    assert not _differs(R.search(oracle, slab, index, q, 10, 1)[0], R.search(oracle, slab, index, q, 10, 1, rules={"stride_k_tiles"})[0])
    # the slots after an empty probed list dropped: the duplicate corpus, whose empty twin is the second list probed — at nprobe 4
    # the 50 rows of the third list are lost, and k = 64 is no longer filled
    slab, nlist = CS.duplicate_corpus()
    for iters in (0, 1):
        index = R.build(oracle, slab, nlist, iters)
        for q in CS.duplicate_queries():
            good, bad = R.search(oracle, slab, index, q, 64, 4), R.search(oracle, slab, index, q, 64, 4, rules={"stop_at_empty"})
            assert (good[2], bad[2]) == (R.APPROXIMATE, R.UNDERFILLED)
    q = CS.duplicate_queries()[5]
    good, bad = R.search(oracle, slab, index, q, 100, 128), R.search(oracle, slab, index, q, 100, 128, rules={"stop_at_empty"})
    assert _differs(good[0], bad[0]) or good[2] != bad[2]
    # the assignment's second launch left out: the rows from 2^20 on are in no list
    slab, live, nlist = CS.two_launch_corpus()
    good, bad = R.build(oracle, slab, nlist, 0), R.build(oracle, slab, nlist, 0, rules={"first_launch"})
    assert good.rows.size - bad.rows.size == slab.shape[0] - CS.IVF_LAUNCH_ROWS and (good.offsets != bad.offsets).any()


# ---- the caps ----

def test_the_caps_are_kernels_hpp_constants():
    text = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "kernels.hpp")).read()

    def const(name):
        m = re.search(r"\b" + name + r"\s*=\s*([0-9 *<u]+)[;,]", text)
        assert m, name
        return int(eval(m.group(1).replace("u", "").replace("<<", " << ")))
    assert const("kGatherMaxK") == CS.GATHER_MAX_K and const("kGatherTileRows") == CS.GATHER_TILE_ROWS
    assert const("kGatherLdsBudget") == CS.GATHER_LDS_BUDGET
    assert (const("kIvfMaxLists"), const("kIvfMaxProbe"), const("kIvfMaxIters")) == (CS.MAX_LISTS, CS.MAX_PROBE, CS.MAX_ITERS)
    assert const("kIvfMergeMaxEntries") == CS.MERGE_MAX_ENTRIES == 16384
    src = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "filter_gather_kernels.hip")).read()
    assert "(row_bytes + 255u - 64u) / 256u * 256u + 64u" in src and "kWavesPerBlock * (2 * (size_t)kcap) * 8" in src
    # the LDS formula: 64 rows 64 bytes apart modulo 256, a query and 2 x kcap entries per wave, the row ids
    assert CS.gather_lds_bytes(384, 64) == 64 * 832 + 4 * 384 * 4 + 4 * 128 * 8 + 256
    assert CS.gather_supported(384, 10) and CS.gather_supported(384, 256) and CS.gather_supported(64, 65)
    assert not CS.gather_supported(12, 10) and not CS.gather_supported(384, 257) and not CS.gather_supported(4, 1)
    top64 = max(d for d in range(8, 4096, 8) if CS.gather_supported(d, 64))
    top256 = max(d for d in range(8, 4096, 8) if CS.gather_supported(d, 256))
    assert CS.gather_lds_bytes(top64, 64) <= CS.GATHER_LDS_BUDGET < CS.gather_lds_bytes(top64 + 8, 64) and top256 <= top64
    # the per-call limits
    assert CS.call_ok(64, 64, 256, 64) and not CS.call_ok(64, 128, 256, 65)      # nprobe * k <= 16,384
    assert CS.call_ok(64, 300, 64, 256) and not CS.call_ok(64, 300, 64, 257)     # nprobe <= 256
    assert not CS.call_ok(64, 4, 10, 5)                                          # nprobe <= nlist

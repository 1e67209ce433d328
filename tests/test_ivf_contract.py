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

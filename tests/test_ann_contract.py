"""The graph ANN search's contract without a GPU: tests/ann_ref.py — the pure function the device must reproduce — is held to the CPU
oracle, to hand-written traces and to each rule on its own; the recall certificates, in ann_ref and in the library's host functions,
are held to hand-computed values."""
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ann_ref as R  # noqa: E402

PAD = R.PAD
F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def all_scores(oracle, slab_u16, q, hreduce=0):
    return oracle.gather_dot(slab_u16, q, np.arange(slab_u16.shape[0], dtype=np.uint32), hreduce)


# ---- the search ----

def test_every_row_an_entry_row_is_the_exact_search_for_any_graph(oracle):
    rng = np.random.default_rng(1)
    n, dim = 500, 64
    slab = R.unit_rows(rng, n, dim).astype(np.float16).view(np.uint16)
    live = rng.random(n) > 0.1
    junk = rng.integers(0, n + 50, size=(n, 5), dtype=np.uint32)   # some ids past the index, no structure at all
    junk[rng.random((n, 5)) < 0.1] = PAD
    for qi in range(6):
        q = R.unit_rows(rng, 1, dim)[0]
        sc = all_scores(oracle, slab, q)
        for k, ef in ((1, 1), (10, 10), (10, 64), (256, 256)):
            want_rows, want_scores = oracle.search_top_k(slab, q, k, live=live)
            rows, scores, count, scored, _ = R.search(sc, live, junk, k, ef, n_entry=n)
            assert count == len(want_rows) and scored == int(live.sum())
            assert (rows == want_rows).all() and (bits(scores) == bits(want_scores)).all()


def chain():
    """Eight rows in a chain: list i = [i + 1, i - 1], a missing end is a pad.  Scores rise with the row."""
    g = np.full((8, 2), PAD, dtype=np.uint32)
    for i in range(8):
        if i + 1 < 8:
            g[i, 0] = i + 1
        if i >= 1:
            g[i, 1] = i - 1
    return g, np.arange(1, 9, dtype=F32) / 10


def test_chain_graph_beam_after_every_step_by_hand():
    g, sc = chain()
    trace = []
    rows, scores, count, scored, steps = R.search(sc, None, g, 2, 2, n_entry=1, expand=1, trace=trace)
    # entry row 0; every step expands the best unexpanded entry i and admits i + 1 (i - 1 is visited); row 7's list opens with a pad
    assert trace == [[0], [1, 0], [2, 1], [3, 2], [4, 3], [5, 4], [6, 5], [7, 6], [7, 6]]
    assert (rows == [7, 6]).all() and (bits(scores) == bits(sc[[7, 6]])).all()
    assert (count, scored, steps) == (2, 8, 8)   # a ninth step finds 7 and 6 both expanded: the search stops
    # up to two entries per step, but only one is ever unexpanded: 0 -> 1; 1 -> 2 (0 is visited); 2 -> 3 ...
    trace = []
    R.search(sc, None, g, 3, 3, n_entry=1, expand=2, trace=trace)
    assert trace[:4] == [[0], [1, 0], [2, 1, 0], [3, 2, 1]]
    # entry rows 0 and 4 (floor(i * 8 / 2)): the beam starts [4, 0]; step 1 expands both: 5, 3 and 1 are admitted
    trace = []
    R.search(sc, None, g, 4, 4, n_entry=2, expand=2, trace=trace)
    assert trace[0] == [4, 0] and trace[1] == [5, 4, 3, 1]
    # step 2 expands 5 and 3: 6 and 2 are admitted (4 is visited); best four of {5, 4, 3, 1, 6, 2}
    assert trace[2] == [6, 5, 4, 3]


def test_max_iters_cuts_the_walk():
    g, sc = chain()
    rows, _, count, scored, steps = R.search(sc, None, g, 2, 2, n_entry=1, expand=1, max_iters=3)
    assert (rows == [3, 2]).all() and (count, scored, steps) == (2, 4, 3)


def test_a_pad_ends_the_list_and_degree_cuts_it():
    sc = np.asarray([0.1, 0.9, 0.5, 0.7], dtype=F32)
    g = np.asarray([[PAD, 1, 2], [PAD, PAD, PAD], [PAD, PAD, PAD], [PAD, PAD, PAD]], dtype=np.uint32)
    rows, _, count, scored, steps = R.search(sc, None, g, 4, 4, n_entry=1)
    assert (rows == [0]).all() and (count, scored, steps) == (1, 1, 1)     # rows 1 and 2 lie behind the pad
    g[0] = [2, 1, 3]
    rows, _, count, _, _ = R.search(sc, None, g, 4, 4, n_entry=1, degree=2)
    assert (rows == [1, 2, 0]).all() and count == 3                         # column 2 (row 3) is past the degree
    rows, _, count, _, _ = R.search(sc, None, g, 4, 4, n_entry=1)
    assert (rows == [1, 3, 2, 0]).all() and count == 4
    g[0] = [2, 9, 1]                                                         # an id past the index is skipped, the walk goes on
    rows, _, _, _, _ = R.search(sc, None, g, 4, 4, n_entry=1)
    assert (rows == [1, 2, 0]).all()
    rows, _, _, _, _ = R.search(sc, None, g + np.uint32(100) * (g != PAD), 4, 4, n_entry=1, row_base=100)
    assert (rows == [101, 102, 100]).all()                                   # ids are global; 109 is outside 100 .. 103


def test_tombstoned_rows_are_never_admitted():
    g, sc = chain()
    live = np.ones(8, dtype=bool)
    live[3] = False                              # the chain is cut: nothing above row 2 is reachable from row 0
    rows, _, count, scored, _ = R.search(sc, live, g, 8, 8, n_entry=1, expand=1)
    assert (rows == [2, 1, 0]).all() and (count, scored) == (3, 3)
    live[:] = True
    live[0] = False                              # entry rows 0 and 4: only 4 is scored; 0 is reachable from 1 and stays out
    rows, _, count, scored, _ = R.search(sc, live, g, 8, 8, n_entry=2, expand=2)
    assert (rows == [7, 6, 5, 4, 3, 2, 1]).all() and (count, scored) == (7, 7)
    live[:] = False
    assert R.search(sc, live, g, 8, 8, n_entry=8)[2] == 0


def test_underfill_detection():
    assert R.flag_of(10, 10, 4096) == R.APPROXIMATE
    assert R.flag_of(3, 10, 3) == R.APPROXIMATE           # only three live rows exist
    assert R.flag_of(3, 10, 4) == R.UNDERFILLED
    assert R.flag_of(0, 10, 4) == R.EMPTY_DESPITE_INDEXED_POINTS
    assert R.flag_of(0, 10, 0) == R.APPROXIMATE           # nothing live: count 0 is the answer
    g = np.full((8, 2), PAD, dtype=np.uint32)             # an all-pad table: only the entry rows are ever seen
    count = R.search(chain()[1], None, g, 6, 6, n_entry=4)[2]
    assert count == 4 and R.flag_of(count, 6, 8) == R.UNDERFILLED


# ---- the certificates ----

def _both():
    """ann_ref and the library's host functions (no device needed), under one signature."""
    from frankensearch_amd.build import build
    build()
    from frankensearch_amd import ann as A

    def lib_min(fn):
        def run(cal, target, level):
            c = fn(cal, target, level)
            return None if c is None else (c.ef_search, c.certified_recall, c.meets_target)
        return run
    ref = dict(conformal=R.conformal_recall_lower_bound, hoeffding=R.mean_recall_lower_bound,
               bernstein=R.mean_recall_lower_bound_bernstein, min_ef=R.certified_min_ef, min_ef_mean=R.certified_min_ef_mean)
    lib = dict(conformal=A.conformal_recall_lower_bound, hoeffding=A.mean_recall_lower_bound,
               bernstein=A.mean_recall_lower_bound_bernstein, min_ef=lib_min(A.certified_min_ef),
               min_ef_mean=lib_min(A.certified_min_ef_mean))
    return [("ann_ref", ref), ("library", lib)]


def test_conformal_bound_by_hand():
    sample = [0.95, 0.4, 1.0, 0.7, 0.9, 0.8, 1.0, 0.6, 1.0, 0.85, 0.9, 1.0, 0.75, 1.0, 0.9, 1.0, 0.5, 1.0, 0.9]
    assert len(sample) == 19
    for name, f in _both():
        assert f["conformal"](sample, 0.1) == 0.5, name              # floor(0.1 * 20) = 2: the 2nd smallest
        assert f["conformal"](sample, 0.05) == 0.4, name             # rank 1
        assert f["conformal"](sample[:10], 0.05) == 0.0, name        # floor(0.05 * 11) = 0: nothing to certify
        assert f["conformal"](sample + [float("nan"), float("inf")], 0.1) == 0.5, name   # non-finite entries are ignored
        assert f["conformal"]([2.0] * 19 + [-1.0], 0.05) == 0.0, name                    # -1 clamps to 0 ...
        assert f["conformal"]([2.0] * 19, 0.1) == 1.0, name                              # ... and 2 to 1
        for alpha in (0.0, 1.0, -0.1, 1.5, float("nan")):
            assert f["conformal"](sample, alpha) == 0.0, (name, alpha)
        assert f["conformal"]([], 0.1) == 0.0, name


def test_mean_bounds_closed_forms():
    const = [0.9] * 50
    two = [1.0] * 30 + [0.5] * 10
    for name, f in _both():
        want = 0.9 - math.sqrt(math.log(1.0 / 0.05) / 100.0)
        assert abs(f["hoeffding"](const, 0.05) - want) < 1e-12, name
        assert f["hoeffding"]([0.1] * 4, 0.05) == 0.0, name          # 0.1 - 0.61 clamps to 0
        assert f["hoeffding"](const, 1.0) == 0.0 and f["hoeffding"]([], 0.05) == 0.0, name
        # a constant sample has no variance: only the 7 ln(2 / delta) / (3 (n - 1)) term is left
        want = 0.9 - 7.0 * math.log(2.0 / 0.05) / (3.0 * 49.0)
        assert abs(f["bernstein"](const, 0.05) - want) < 1e-9, name
        # mean 0.875, unbiased variance 30 * 0.125^2 + 10 * 0.375^2 over 39 = 1.875 / 39
        ln = math.log(2.0 / 0.1)
        want = 0.875 - math.sqrt(2.0 * (1.875 / 39.0) * ln / 40.0) - 7.0 * ln / (3.0 * 39.0)
        assert abs(f["bernstein"](two, 0.1) - want) < 1e-12, name
        assert f["bernstein"]([0.9], 0.05) == 0.0 and f["bernstein"](two, 1.0) == 0.0, name
        assert f["bernstein"](two + [float("nan")], 0.1) == f["bernstein"](two, 0.1), name


def test_certified_min_ef_picks_the_smallest_qualifying_ef_and_otherwise_the_best():
    lo, mid, hi = [0.5] * 19, [0.9] * 19, [1.0] * 19
    for name, f in _both():
        assert f["min_ef"]([(128, hi), (16, lo), (64, mid), (32, mid)], 0.9, 0.1) == (32, 0.9, True), name
        assert f["min_ef"]([(128, mid), (16, lo), (64, mid)], 0.95, 0.1) == (64, 0.9, False), name   # the first of the best
        assert f["min_ef"]([], 0.9, 0.1) is None, name
        got = f["min_ef_mean"]([(16, lo), (32, hi)], 0.6, 0.1)      # 0.5 - 0.388 misses, 1.0 - 0.388 meets
        assert got[0] == 32 and got[2] and abs(got[1] - (1.0 - 7.0 * math.log(20.0) / 54.0)) < 1e-12, name


def test_calibrate_measures_only_up_to_the_chosen_ef():
    asked = []

    def measure(ef):
        asked.append(ef)
        return [min(1.0, ef / 64.0)] * 19
    chosen, sweep = R.calibrate([128, 16, 64, 32, 64, 256], measure, 0.9, 0.1)
    assert asked == [16, 32, 64] and chosen == (64, 1.0, True)
    assert sweep == [(16, 0.25, False), (32, 0.5, False), (64, 1.0, True)]
    asked.clear()
    chosen, sweep = R.calibrate([16, 32], measure, 0.9, 0.1)
    assert asked == [16, 32] and chosen == (32, 0.5, False) and len(sweep) == 2
    assert R.calibrate([], measure, 0.9, 0.1) is None
    assert R.recall_at_k_of([1, 2, 3], [3, 4]) == 0.5 and R.recall_at_k_of([], []) == 1.0 and R.recall_sample([3, 4], 1, [3, 4]) == 0.0


# ---- the fixture is approximate ----

def test_iid_rows_make_the_search_truly_approximate(oracle):
    rng = np.random.default_rng(7)
    n, dim, m, k = 4096, 64, 16, 10
    vec = R.unit_rows(rng, n, dim).astype(np.float16)
    slab = vec.view(np.uint16)
    table = R.knn_table(vec.astype(F32), m)
    queries = R.unit_rows(rng, 24, dim)
    recall = {16: [], 128: []}
    differing = 0
    for q in queries:
        sc = all_scores(oracle, slab, q)
        exact, _ = oracle.search_top_k(slab, q, k)
        for ef in recall:
            rows, _, count, _, _ = R.search(sc, None, table, k, ef, n_entry=256)
            assert count == k
            recall[ef].append(R.recall_at_k_of(rows, exact))
            if ef == 16 and list(rows) != list(exact):
                differing += 1
    lo, hi = float(np.mean(recall[16])), float(np.mean(recall[128]))
    print(f"recall@10 over {len(queries)} iid queries: ef 16 {lo:.3f}, ef 128 {hi:.3f}; differing from exact at ef 16: {differing}")
    assert differing >= 1
    assert hi > lo


# ---- the hand-made cases of test_gpu_ann_shapes.py can see the mistakes they aim at ----

import ann_cases as C  # noqa: E402


def test_a_plain_left_to_right_dot_differs_from_the_oracle_at_every_dot_dimension(oracle):
    """The dot cases compare score BITS, which only proves the kernel's accumulation order if another order gives other bits on the
    very rows and queries the GPU test uses.  Share of (query, row) pairs whose plain left-to-right f32 dot differs from the oracle's,
    printed per dimension; above dimension 8 it must not be zero.  Up to 8 there is at most one chunk — one product per accumulator
    and the horizontal add, or the fused tail alone — and the share is whatever it is: printed, not asserted."""
    for f32, dims in ((False, list(C.F16_VECTOR_DIMS) + list(C.F16_ELEMENT_DIMS)), (True, list(C.F32_VECTOR_DIMS) + list(C.F32_ELEMENT_DIMS))):
        for dim in sorted(dims):
            c = C.dot_case(dim, f32)
            want = C.score_table(oracle, c["slab"], c["queries"], f32, 0)
            share = float((bits(C.plain_dot(c["slab"], c["queries"], f32)) != bits(want)).mean())
            print(f"{'f32' if f32 else 'f16'} slab, dimension {dim}: plain dot differs in {share:.4f} of the scores")
            if dim > 8:
                assert share > 0.0, (f32, dim)


def _answers(c, scores, k, ef, cfg, mutation):
    return [C.mutated_search(scores[i], c["live"], c["table"], k, ef, mutation, row_base=c["row_base"], **cfg)
            for i in range(len(c["queries"]))]


def _changed(c, scores, k, ef, cfg, mutation):
    """Queries whose answer (rows, in order) differs under the mutation."""
    a, b = _answers(c, scores, k, ef, cfg, None), _answers(c, scores, k, ef, cfg, mutation)
    return [i for i in range(len(a)) if a[i][2] != b[i][2] or (a[i][0] != b[i][0]).any()]


def test_the_restated_search_without_a_mutation_is_ann_ref(oracle):
    c = C.hostile_case(1000)
    scores = C.score_table(oracle, c["slab"], c["queries"], False, 0)
    for cfg in C.HOSTILE_CFGS:
        for i in range(C.NQ):
            rows, sc, count = C.mutated_search(scores[i], c["live"], c["table"], 10, 64, None, row_base=1000, **cfg)
            wr, ws, wc, _, _ = R.search(scores[i], c["live"], c["table"], 10, 64, row_base=1000, **cfg)
            assert count == wc and (rows == wr).all() and (bits(sc) == bits(ws)).all()


def test_each_broken_rule_changes_an_answer_of_the_case_that_aims_at_it(oracle):
    for row_base in (0, 1000):
        c = C.hostile_case(row_base)
        scores = C.score_table(oracle, c["slab"], c["queries"], False, 0)
        for k, ef in C.K_EF:
            for cfg in C.HOSTILE_CFGS:
                pad = _changed(c, scores, k, ef, cfg, "walk past a pad")
                dup = _changed(c, scores, k, ef, cfg, "no de-duplication within a step")
                print(f"hostile table, row_base {row_base}, k {k} ef {ef} {cfg}: walking past a pad changes queries {pad}, no de-duplication {dup}")
                assert pad and dup
                if (k, ef) == (10, 64):   # a walk long enough to meet them: Y0 surfaces in query 1's answer, X0 twice in query 0's
                    assert 1 in pad and 0 in dup
    for identical in (False, True):
        c = C.tie_case(identical)
        scores = C.score_table(oracle, c["slab"], c["queries"], False, 0)
        for k, ef in C.TIE_K_EF:
            tie = _changed(c, scores, k, ef, dict(n_entry=C.N_ENTRY), "ties by row descending")
            print(f"ties (identical rows {identical}), k {k} ef {ef}: row-descending ties change {len(tie)} of {C.NQ} queries")
            assert tie
    for f32 in (False, True):
        c = C.nonfinite_case(f32)
        scores = C.score_table(oracle, c["slab"], c["queries"], f32, 0)
        for cfg, (k, ef) in C.NONFINITE_CFGS:
            nan = _changed(c, scores, k, ef, cfg, "NaN above +inf")
            print(f"non-finite scores (f32 {f32}), k {k} ef {ef} {cfg}: NaN above +inf changes {len(nan)} of {C.NQ} queries")
            assert nan


def test_non_finite_case_brings_every_kind_of_score_into_the_answers(oracle):
    for f32 in (False, True):
        c = C.nonfinite_case(f32)
        scores = C.score_table(oracle, c["slab"], c["queries"], f32, 0)
        kinds = set()
        for cfg, (k, ef) in C.NONFINITE_CFGS:
            for i in range(C.NQ):
                _, sc, count, _, _ = R.search(scores[i], c["live"], c["table"], k, ef, **cfg)
                assert R.flag_of(count, k, int(c["live"].sum())) == R.APPROXIMATE
                kinds |= {"nan"} if np.isnan(sc).any() else set()
                kinds |= {"+inf"} if np.isposinf(sc).any() else set()
                kinds |= {"-inf"} if np.isneginf(sc).any() else set()
        assert kinds == {"nan", "+inf", "-inf"}, (f32, kinds)


def test_visited_table_rows_for_the_chain_case():
    picked = C.chain_rows()
    h = ((picked.astype(np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)
    assert picked.size >= 40 and set(h.tolist()) == {8190, 8191}
    assert not set(R.entry_rows(C.CHAIN_N, 1)) & set(picked.tolist())       # n_entry = 1: row 0 alone
    c = C.chain_case()
    assert set(c["table"][0].tolist()) <= set(picked.tolist()) and len(set(c["table"][0].tolist())) == C.WIDTH
    for p in picked:
        assert set(c["table"][p].tolist()) <= set(picked.tolist()) - {int(p)}
    assert (np.delete(c["table"], np.concatenate([[0], picked]), axis=0) == PAD).all()


def test_lds_boundary_dimensions_follow_from_the_kernel_constants():
    """ann_cases.ANN_STATE_BYTES restates the kOff* layout of ann_kernels.hip; the constants it is built from are read back from
    kernels.hpp here, so a changed limit shows up as a failure of this test rather than as a test that silently lost its boundary."""
    import re
    text = open(os.path.join(ROOT, "frankensearch_amd", "csrc", "kernels.hpp")).read()
    const = {m.group(1): int(m.group(2)) for m in re.finditer(r"constexpr uint32_t (kAnn\w+) = (\d+);", text)}
    assert (const["kAnnMaxEf"], const["kAnnMaxStepRows"], const["kAnnTableSlots"], const["kAnnMaxDim"]) == (256, 512, 8192, C.ANN_MAX_DIM)
    assert C.ANN_STATE_BYTES == 45664
    assert C.ann_lds_bytes(4968) == 64 * 1024 and C.ann_lds_bytes(4969) == 64 * 1024 + 16 and C.ann_lds_bytes(4976) > 64 * 1024
    assert C.ann_lds_bytes(C.ANN_MAX_DIM) == 111200 <= 160 * 1024

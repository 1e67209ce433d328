"""The graph ANN search (ann_kernels.hip) at the shapes, tables and scores that test_gpu_ann.py's random rows over built tables never
reach.  Same contract, same references: rows, score bits, counts, flags, rows_scored and steps of tests/ann_ref.py over the CPU oracle's
scores, no tolerance.  Every table is made by hand (tests/ann_cases.py), so no k-NN build limits the dimension.

  a, b  every form of the two dots: vector and element loads, no group, leftover chunks, tails, more groups than one batch of loads
  c     a query + state past 64 KB of LDS (the hipFuncSetAttribute branch of ann_prepare), up to the largest dimension accepted
  d     a table that is wrong in every way a table can be: nothing it names may become an address unchecked
  e     probe chains of the visited table that run past its last slot
  f, g  ties on the score everywhere; +inf, -inf and NaN scores beside the kEmpty padding of a step's sort
  h     indexes of 1, 2 and 17 rows; flags and the exact fallback
test_ann_contract.py shows, without a GPU, that each of these cases answers differently when the rule it aims at is broken."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ann_cases as C  # noqa: E402
import ann_ref as R  # noqa: E402
from ann_cases import assert_device_is_reference, bits, score_table  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = R.PAD


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    return fa_mod


def make_index(fa, c, hreduce=0):
    make = fa.VectorIndex.from_slab_f32 if c["f32"] else fa.VectorIndex.from_slab
    idx = make(c["slab"], live=c["live"], row_base=c["row_base"])
    idx.set_hreduce(hreduce)
    return idx


def run(fa, oracle, c, runs, hreduce=0, what=""):
    """runs: (config, ((k, ef), ...)) pairs, all on one index and one oracle score table -> that table."""
    idx = make_index(fa, c, hreduce)
    scores = score_table(oracle, c["slab"], c["queries"], c["f32"], hreduce)
    for cfg, pairs in runs:
        ann = fa.AnnIndex(idx, c["table"], fa.AnnConfig(**cfg))
        for k, ef in pairs:
            assert_device_is_reference(ann, c["table"], scores, c["live"], c["queries"], k, ef, cfg, c["row_base"], what)
    return scores


def same_scores(got, want):
    """NaN where the reference has a NaN (payload and sign are the platform's), the reference's bits everywhere else."""
    nan = np.isnan(want)
    return bool(np.isnan(got[nan]).all() and (bits(got[~nan]) == bits(want[~nan])).all())


def assert_device_is_reference_or_exact(ann, idx, c, scores, k, ef, cfg, what):
    """assert_device_is_reference for cases with NaN scores and for answers the beam leaves short: the flag is R.flag_of of the
    reference's count, a flagged query carries the exact batched search's answer, the counters count the beam's work either way."""
    queries, live, table = c["queries"], c["live"], c["table"]
    rows, sc, counts, flags = ann.search_batched(queries, k, ef)
    st = ann.stats
    exact = None
    live_rows = int(live.sum()) if live is not None else scores.shape[1]
    want_scored = want_steps = 0
    seen = {R.APPROXIMATE: 0, R.UNDERFILLED: 0, R.EMPTY_DESPITE_INDEXED_POINTS: 0}
    for i in range(len(queries)):
        wr, ws, wc, scored, steps = R.search(scores[i], live, table, k, ef, row_base=c["row_base"], **cfg)
        want_scored += scored
        want_steps += steps
        flag = R.flag_of(wc, k, live_rows)
        seen[flag] += 1
        assert flags[i] == flag, (what, i, flags[i], flag)
        if flag != R.APPROXIMATE:
            exact = exact or idx.search_batched(queries, k)
            er, es, ec = exact[:3]
            wr, ws, wc = er[i, :ec[i]], es[i, :ec[i]], int(ec[i])
        assert counts[i] == wc and (rows[i, :wc] == wr).all() and same_scores(sc[i, :wc], ws), (what, i, rows[i], wr)
    print(f"{what}: k {k} ef {ef} {cfg}: flags {seen}, rows scored {st.rows_scored}, steps {st.steps}")
    assert (st.rows_scored, st.steps) == (want_scored, want_steps)
    assert (st.approximate, st.underfilled, st.empty_despite_indexed_points) == tuple(seen[f] for f in (0, 1, 2))
    return seen


def orders(dims):
    return [(d, h) for i, d in enumerate(dims) for h in ((0, 1, 2) if d in C.ALL_HREDUCE_DIMS else (i % 3,))]


# ---- a, b: the dot forms ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,hreduce", orders(list(C.F16_VECTOR_DIMS) + list(C.F16_ELEMENT_DIMS)))
def test_f16_dot_forms(fa, oracle, dim, hreduce):
    c = C.dot_case(dim, f32=False)
    run(fa, oracle, c, [(dict(n_entry=C.N_ENTRY), C.K_EF)], hreduce, f"f16 dim {dim} hreduce {hreduce}")


@pytest.mark.parametrize("dim,hreduce", [(d, i % 3) for i, d in enumerate(list(C.F32_VECTOR_DIMS) + list(C.F32_ELEMENT_DIMS))])
def test_f32_dot_forms(fa, oracle, dim, hreduce):
    c = C.dot_case(dim, f32=True)
    assert (c["slab"] != c["slab"].astype(np.float16).astype(np.float32)).mean() > 0.9   # not f16 values
    run(fa, oracle, c, [(dict(n_entry=C.N_ENTRY), C.K_EF)], hreduce, f"f32 dim {dim} hreduce {hreduce}")


# ---- c: LDS past 64 KB -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim,f32", [(d, False) for d in C.LDS_DIMS] + [(4976, True)])
def test_query_and_state_past_64_kb_of_lds(fa, oracle, dim, f32):
    """4,968 is the last dimension whose query + state fit 64 KB exactly, 4,976 the first multiple of 8 past it (ann_cases.py derives
    both), 16,384 is kAnnMaxDim — the index itself sets no limit on the dimension, so the largest case IS the ANN search's largest."""
    assert C.ann_lds_bytes(4968) == 65536 and C.ann_lds_bytes(4969) > 65536 and C.ann_lds_bytes(C.ANN_MAX_DIM) == 111200
    c = C.dot_case(dim, f32, n=C.LDS_N, nq=C.LDS_NQ)
    run(fa, oracle, c, [(dict(n_entry=C.N_ENTRY), C.K_EF)], 0, f"lds {C.ann_lds_bytes(dim)} bytes, dim {dim} f32 {f32}")
    if dim == C.ANN_MAX_DIM:   # one dimension more is refused at create, before anything is launched
        over = fa.VectorIndex.from_slab(np.zeros((4, dim + 8), dtype=np.uint16))
        with pytest.raises(fa.InvalidConfig):
            fa.AnnIndex(over, np.full((4, 2), PAD, dtype=np.uint32), fa.AnnConfig(n_entry=1))


# ---- d: hostile tables -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("row_base", [0, 1000])
def test_hostile_table(fa, oracle, row_base):
    """The walk and admit loops of ann_search_kernel, re-read for this test: `parent < n` guards the table read (parents are beam
    rows, admitted below n); an id becomes `row = id - row_base`, which wraps for ids below the base, and `row >= n` is tested before
    the live bit, the entry test and the hash table see it; admit[] and cand[] are indexed by counters capped at kAnnMaxStepRows; the
    score pass tests `row >= n` again.  So this table can only produce a wrong answer, never a wild address."""
    c = C.hostile_case(row_base)
    scores = run(fa, oracle, c, [(cfg, C.K_EF) for cfg in C.HOSTILE_CFGS], 0, f"hostile table, row_base {row_base}")
    idx = make_index(fa, c)
    ann = fa.AnnIndex(idx, c["table"], fa.AnnConfig(n_entry=C.N_ENTRY))
    rows, _, counts, _ = ann.search_batched(c["queries"], 10, 64)
    assert rows[0, 0] == c["x0"] + row_base            # named by every list, admitted once
    assert (rows[0] == c["x0"] + row_base).sum() == 1
    assert c["y0"] + row_base not in rows               # named only behind pads
    assert int(np.argmax(scores[1])) == c["y0"]         # ... and it would have led query 1's answer


# ---- e: the visited table's chains ------------------------------------------------------------------------------------------------------

def test_visited_table_chains_run_past_the_last_slot(fa, oracle):
    """Every row the steps can reach hashes to slot 8,190 or 8,191 of the 8,192-slot visited table, so after the first two the
    insertions probe on through slot 0: the `& (kAnnTableSlots - 1)` wrap.  The reference keeps a Python set and knows no slots.
    The rows are picked with the kernel's hash as it stands (ann_cases.chain_rows); if the kernel's hash ever changes this test
    stays correct but loses its point — re-derive chain_rows then."""
    c = C.chain_case()
    picked = c["picked"]
    assert picked.size >= 40 and 0 not in picked        # row 0 is the one entry row
    scores = run(fa, oracle, c, [(dict(n_entry=1), C.K_EF)], 0, "visited-table chains")
    # the first step alone admits 16 rows of two home slots: at least 8 share one, and two slots hold them no longer
    _, _, _, scored, _ = R.search(scores[0], None, c["table"], 10, 64, n_entry=1)
    assert scored >= 1 + C.WIDTH


# ---- f, g: ties and non-finite scores ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("identical", [False, True])
def test_ties_everywhere(fa, oracle, identical):
    c = C.tie_case(identical)
    scores = run(fa, oracle, c, [(dict(n_entry=C.N_ENTRY), C.TIE_K_EF)], 0, f"ties, identical rows {identical}")
    assert all(np.unique(bits(s)).size <= (1 if identical else 16) for s in scores)


@pytest.mark.parametrize("f32", [False, True])
def test_non_finite_scores(fa, oracle, f32):
    c = C.nonfinite_case(f32)
    idx = make_index(fa, c)
    scores = score_table(oracle, c["slab"], c["queries"], f32, 0)
    s = scores[:, c["live"]]
    assert np.isposinf(s[:6]).any(axis=1).all() and np.isneginf(s[:6]).any(axis=1).all() and np.isnan(s).any(axis=1).all()
    nan_answers = 0
    for cfg, (k, ef) in C.NONFINITE_CFGS:
        ann = fa.AnnIndex(idx, c["table"], fa.AnnConfig(**cfg))
        seen = assert_device_is_reference_or_exact(ann, idx, c, scores, k, ef, cfg, f"non-finite scores, f32 {f32}")
        assert seen[R.APPROXIMATE] == C.NQ
        nan_answers += int(np.isnan(ann.search_batched(c["queries"], k, ef)[1]).any())
    assert nan_answers   # NaN scores do reach the answers (k 224 of about 235 rows scored)


# ---- h: tiny indexes ---------------------------------------------------------------------------------------------------------------------

def tiny(n, table, live=None, seed=5):
    rng = np.random.default_rng(seed)
    half = R.unit_rows(rng, n, 64).astype(np.float16)
    return dict(slab=half.view(np.uint16), queries=R.unit_rows(rng, 5, 64), live=live, table=np.asarray(table, dtype=np.uint32), f32=False,
                row_base=0)


def test_tiny_indexes_flags_and_the_exact_fallback(fa, oracle):
    ring = [[(i + 1) % 17, (i + 5) % 17, i, PAD] for i in range(17)]
    dead = np.ones(17, dtype=bool)
    dead[[3, 9]] = False
    star = [[1, 2, 3, PAD]] + [[PAD] * 4] * 16          # row 0 reaches three rows, nothing leads on
    no_entry = np.ones(17, dtype=bool)
    no_entry[0] = False
    cases = [
        ("1 row", tiny(1, [[0, PAD]]), dict(n_entry=1), ((1, 1), (1, 16), (10, 64)), R.APPROXIMATE),
        ("2 rows", tiny(2, [[1, 0], [0, 1]]), dict(n_entry=1), ((1, 16), (2, 16), (10, 64)), R.APPROXIMATE),
        ("17 rows", tiny(17, ring, dead), dict(n_entry=1, expand=1), ((10, 16), (16, 16), (17, 256), (256, 256)), R.APPROXIMATE),
        ("17 entry rows", tiny(17, ring, dead), dict(n_entry=17), ((10, 16), (16, 256)), R.APPROXIMATE),
        ("n_entry past the rows", tiny(17, ring), dict(n_entry=1024), ((17, 17),), R.APPROXIMATE),
        ("underfilled", tiny(17, star, dead), dict(n_entry=1), ((10, 16), (10, 256)), R.UNDERFILLED),
        ("no live entry row", tiny(17, star, no_entry), dict(n_entry=1), ((10, 16),), R.EMPTY_DESPITE_INDEXED_POINTS),
    ]
    for what, c, cfg, pairs, flag in cases:
        idx = make_index(fa, c)
        scores = score_table(oracle, c["slab"], c["queries"], False, 0)
        ann = fa.AnnIndex(idx, c["table"], fa.AnnConfig(**cfg))
        for k, ef in pairs:
            seen = assert_device_is_reference_or_exact(ann, idx, c, scores, k, ef, cfg, what)
            assert seen[flag] == len(c["queries"]), (what, k, ef, seen)

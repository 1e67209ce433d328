"""CPU checks of the MMR contract: fsgpu_mmr_rerank — the host restatement inside libfsgpu.so, which is also the fallback and the
comparator of the device path — against the reference's inline tests (crates/frankensearch-fusion/src/mmr.rs:406-900) and against
tests/mmr_ref.py on random pools: identical order, similarity matrix equal bit for bit.  Config validation and the ABI symbols too."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import mmr_ref as M  # noqa: E402


def _fa():
    import frankensearch_amd as fa
    return fa


def rerank(scores, emb, k, lam=0.7, pool=30, sims=False):
    fa = _fa()
    return fa.mmr_rerank(scores, emb, k, fa.MmrConfig(True, lam, pool), want_sims=sims)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- the reference's inline tests ------------------------------------------------------------------------------------------------
DOC = ([0.9, 0.85, 0.84, 0.5], [[1.0, 0.0, 0.0], [0.99, 0.1, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]])


def test_doc_example_and_first_pick():
    got = rerank(*DOC, 3)
    assert got[0] == 0 and got[1] == 2
    assert rerank([0.5, 0.9, 0.7], np.eye(3), 1).tolist() == [1]


def test_lambda_one_is_pure_relevance_and_zero_is_pure_diversity():
    assert rerank(*DOC, 4, lam=1.0).tolist() == [0, 1, 2, 3]
    got = rerank([0.9, 0.5, 0.8], [[1.0, 0.0], [0.0, 1.0], [0.99, 0.1]], 3, lam=0.0)
    assert got[0] == 0 and got[1] == 1


def test_diversity_penalizes_near_duplicates_and_low_lambda():
    got = rerank(*DOC, 3, lam=0.5)
    assert got[0] == 0 and got[1] == 2
    got = rerank([1.0, 0.9, 0.8, 0.7], [[1.0, 0.0], [0.95, 0.05], [0.0, 1.0], [0.05, 0.95]], 2, lam=0.1)
    assert got[0] == 0 and got[1] in (2, 3)


def test_empty_k_zero_k_greater_than_n_single_candidate():
    assert rerank([], [], 5).size == 0
    assert rerank([1.0], [[1.0, 0.0]], 0).size == 0
    assert rerank([0.9, 0.5], [[1.0, 0.0], [0.0, 1.0]], 10).size == 2
    assert rerank([0.8], [[1.0, 0.0, 0.0]], 1).tolist() == [0]


def test_equal_scores_identical_embeddings_negative_scores():
    assert sorted(rerank([0.5, 0.5, 0.5], np.eye(3), 3, lam=0.5).tolist()) == [0, 1, 2]
    got = rerank([0.9, 0.85, 0.8], [[1.0, 0.0]] * 3, 3, lam=0.5)
    assert got.size == 3 and got[0] == 0
    got = rerank([0.5, 0.5, 0.5], [[1.0, 0.0], [0.0, 1.0], [0.7, 0.7]], 3, lam=0.5)
    assert got.size == 3 and got[0] == 0   # all-equal scores normalise to 1: the first index is the first pick
    got = rerank([-0.1, -0.5, -0.9], np.eye(3), 3)
    assert got[0] == 0 and got.size == 3


def test_candidate_pool_limits_consideration():
    got = rerank([0.9, 0.85, 0.8, 0.7, 0.6], [[1.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.5, 0.5], [0.3, 0.7]], 5, pool=3)
    assert got.size == 3 and all(i < 3 for i in got)


def test_no_duplicates_in_output():
    got = rerank([0.9, 0.88, 0.87, 0.85, 0.84], [[1, 0, 0], [0.9, 0.1, 0], [0, 1, 0], [0, 0.9, 0.1], [0, 0, 1]], 5, lam=0.5)
    assert sorted(got.tolist()) == [0, 1, 2, 3, 4]


def test_cosine_forms_different_lengths_and_zero_vector():
    # a ragged pool takes cosine_sim over the shorter length (mmr.rs:254-279)
    _, s = rerank([1.0, 0.5], [[1.0, 0.0, 0.0, 0.0], [1.0, 0.0]], 2, sims=True)
    assert abs(s[0, 1] - 1.0) < 1e-6
    _, s = rerank([1.0, 0.5, 0.2], [[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [-1.0, 0.0, 0.0]], 3, sims=True)
    assert s[0, 1] == 0.0 and s[0, 0] == 0.0 and abs(s[1, 2] + 1.0) < 1e-6 and abs(s[1, 1] - 1.0) < 1e-6
    _, s = rerank([1.0, 0.5], [[], []], 2, sims=True)
    assert np.all(s == 0.0)


def test_lambda_bounds_and_nan():
    want = {-0.5: 0.0, 1.5: 1.0, math.nan: 0.0, math.inf: 0.0, -math.inf: 0.0}
    rng = np.random.default_rng(3)
    emb = M.clustered(rng, 12, 15, dtype="f32")
    scores = M.scores_for(rng, 12, "plain")
    for lam, clamped in want.items():
        assert M.clamped_lambda(lam) == clamped
        assert rerank(scores, emb, 12, lam=lam).tolist() == rerank(scores, emb, 12, lam=clamped).tolist()
    assert M.clamped_lambda(0.7) == 0.7 and M.clamped_lambda(0.0) == 0.0 and M.clamped_lambda(1.0) == 1.0


def test_norm_hoist_cases_match_the_restatement():
    """mmr.rs incremental_norm_hoist_matches_bruteforce: its xorshift vectors, dims 8 / 64 / 384, n 3 / 16 / 60, k 1 / 5 / n."""
    mask = (1 << 64) - 1
    for dim in (8, 64, 384):
        for n in (3, 16, 60):
            state = 0x2545F4914F6CDD1D ^ ((dim * n) & mask)

            def nxt():
                nonlocal state
                state ^= (state << 13) & mask
                state ^= state >> 7
                state ^= (state << 17) & mask
                return np.float32(np.float32(state >> 40) / np.float32(1 << 24) - np.float32(0.5))
            emb = np.array([[nxt() for _ in range(dim)] for _ in range(n)], dtype=np.float32)
            scores = [(i * 7.0 % 11.0) / 11.0 for i in range(n)]
            for k in (1, 5, n):
                want, _ = M.mmr_rerank(scores, emb, k, 0.55, 1000)
                assert rerank(scores, emb, k, lam=0.55, pool=1000).tolist() == want, (dim, n, k)


# ---- random pools against the restatement --------------------------------------------------------------------------------------
def random_cases():
    rng = np.random.default_rng(20261016)
    dims = (3, 15, 128, 256, 384)
    kinds = ("plain", "ties", "nonfinite", "equal", "negative")
    cases = []
    for i in range(420):
        dim = dims[i % 5]
        if i % 10 == 0:
            n = (1, 2, 30, 128, 127, 64)[(i // 10) % 6]
        else:
            n = int(rng.integers(1, 129)) if i % 3 == 0 else int(rng.integers(2, 41))
        dtype = "f16" if i % 2 == 0 else "f32"
        emb = list(M.clustered(rng, n, dim, dtype=dtype))
        ragged = i % 14 == 5 and n >= 2
        if ragged:   # one document fell back to a shorter (fast-tier) vector
            emb = emb[:12]
            n = len(emb)
            emb[int(rng.integers(0, n))] = M.clustered(rng, 1, max(dim // 2, 1), dtype="f32")[0]
        scores = M.scores_for(rng, n, kinds[(i // 5) % 5])
        lam = (0.7, 0.5, 0.3, 0.0, 1.0, 0.9)[i % 6]
        pool = 30 if i % 4 == 1 else 1000
        k = n if i % 5 else max(1, n // 3)
        cases.append(dict(emb=emb, scores=scores, lam=lam, pool=pool, k=k, dtype=dtype, ragged=ragged, dim=dim))
    return cases


def test_random_pools_match_the_restatement_bit_for_bit():
    cases = random_cases()
    assert len(cases) >= 400
    moved = movable = f32_pools = order_sensitive = ragged = 0
    for c in cases:
        want, want_sims = M.mmr_rerank(list(c["scores"]), c["emb"], c["k"], c["lam"], c["pool"])
        got, got_sims = rerank(c["scores"], c["emb"], c["k"], lam=c["lam"], pool=c["pool"], sims=True)
        assert got.tolist() == want, c
        assert got_sims.shape == want_sims.shape
        same = bits(got_sims) == bits(want_sims)
        both_nan = np.isnan(got_sims) & np.isnan(want_sims)
        assert np.all(same | both_nan), (c["dim"], c["dtype"], int(np.sum(~(same | both_nan))))
        n = want_sims.shape[0]
        ragged += c["ragged"]
        if n >= 3 and c["k"] == min(len(c["emb"]), c["pool"]):
            movable += 1
            moved += want != list(range(len(want)))
        if c["dtype"] == "f32" and not c["ragged"] and c["dim"] >= 15 and n >= 2:
            f32_pools += 1
            E = np.stack(c["emb"][:n])
            order_sensitive += bool(np.any(bits(M.raw_dots(E)) != bits(M.raw_dots(E, accumulators=1))))
    # the cases exercise what they are meant to: MMR moves the order, and the accumulator order shows in the bits of the f32 pools
    assert ragged >= 10
    assert moved * 2 >= movable and movable >= 200, (moved, movable)
    assert order_sensitive * 2 >= f32_pools and f32_pools >= 100, (order_sensitive, f32_pools)


# ---- config and ABI -----------------------------------------------------------------------------------------------------------
def test_config_defaults_and_validation():
    fa = _fa()
    from frankensearch_amd import _lib
    from frankensearch_amd.mmr import _MmrConfig
    d = fa.MmrConfig()
    assert d.enabled is False and d.lambda_ == 0.7 and d.candidate_pool == 30
    c = _MmrConfig(1, 1, 0.0)
    assert _lib.lib().fsgpu_mmr_config_default(C.addressof(c)) == _lib.OK
    assert (c.enabled, c.candidate_pool, c.lambda_, list(c.reserved)) == (0, 30, 0.7, [0, 0, 0, 0])
    assert C.sizeof(_MmrConfig) == 32
    # a bad config is refused before an index handle is looked at: reserved words, enabled beyond 0 / 1
    order = (C.c_uint32 * 4)()
    applied = C.c_uint8(7)
    fake = C.c_void_p(1)   # never dereferenced: the config is checked first
    for bad in (_MmrConfig(2, 30, 0.7), _MmrConfig(1, 30, 0.7, (C.c_uint32 * 4)(0, 0, 1, 0))):
        st = _lib.lib().fsgpu_index_mmr_rerank_docs(fake, None, 0, C.addressof(bad), order, C.byref(applied))
        assert st == _lib.ERR_INVALID_CONFIG and "fsgpu_mmr_config" in _lib.last_error()
        st = _lib.lib().fsgpu_index_mmr_rerank_batched(fake, None, None, None, 0, 1, C.addressof(bad), None, None)
        assert st == _lib.ERR_INVALID_CONFIG
    assert _lib.lib().fsgpu_index_mmr_rerank_docs(None, None, 0, None, order, C.byref(applied)) == _lib.ERR_NULL_ARGUMENT
    cnt = C.c_uint32(9)
    assert _lib.lib().fsgpu_mmr_rerank(None, None, None, 3, 3, 0.7, 30, None, C.byref(cnt), None) == _lib.ERR_NULL_ARGUMENT
    assert cnt.value == 0
    with pytest.raises(ValueError):
        fa.mmr_rerank([1.0], [], 1)


def test_abi_exports_the_mmr_entry_points():
    from frankensearch_amd import _lib
    text = open(os.path.join(ROOT, "include", "fsgpu.h")).read()
    names = ["fsgpu_mmr_config_default", "fsgpu_mmr_rerank", "fsgpu_index_vector_at_f32", "fsgpu_index_mmr_rerank",
             "fsgpu_index_mmr_rerank_batched", "fsgpu_index_mmr_rerank_docs", "fsgpu_two_tier_mmr_rerank"]
    L = C.CDLL(_lib.LIB_PATH)
    for name in names:
        assert name + "(" in text and name in _lib.SIGNATURES and hasattr(L, name), name
    assert "typedef struct fsgpu_mmr_config" in text


def test_mmr_step_is_the_identity_when_disabled_or_short():
    fa = _fa()
    items = [("a", 0.9, 0), ("b", 0.8, 1)]
    assert fa.mmr_step(items, None, fa.MmrConfig()) == (items, False)
    assert fa.mmr_step(items, None, None) == (items, False)
    assert fa.mmr_step(items[:1], None, fa.MmrConfig(True)) == (items[:1], False)


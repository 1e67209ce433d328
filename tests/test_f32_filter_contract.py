"""The int8 filter's certificate over Quantization::F32 rows, on the CPU (no GPU needed).

tests/f32_filter_ref.py restates what the device builds for an F32 slab (scale, int8 rows, E2 / R1 / R2; delta through
oracle/filter_bound.py's restatement of prepare_queries_i8_filter_kernel).  Here that bound is held against

    the real-number dot (float64) of the f32 row and the f32 query, and
    the reference's own f32 score, dot_product_f32_bytes_f32 (simd.rs:581-702), in all three reduce_add orders,

for every (row, query) of the seven corpora of tests/test_gpu_int8_filter.py kept as f32 (never rounded to f16), one corpus spread
over six decades, and the hostile queries.  The last test says, for each case of tests/test_gpu_f32_batched.py's first test, how
many rows sit within the margin of the k-th best integer score: more than the finish's candidate pool (1,024) would make a query
uncertifiable whatever the kernels do, so the GPU test's fallback cap can only hold while this stays below it.
"""
import numpy as np
import pytest

import f32_filter_ref as R

N = 3_000


def corpora(rng, n, dim):
    """tests/test_gpu_int8_filter.py::corpora, as f32 rows."""
    base = R.unit_rows(rng, n, dim)
    yield "gaussian unit rows", base
    out = base.copy()
    out[:, rng.integers(0, dim, 3)] *= 12.0
    yield "outlier dimensions", out / np.linalg.norm(out, axis=1, keepdims=True)
    yield "tiny magnitudes", base * np.float32(3e-3)
    yield "large magnitudes", base * np.float32(180.0)
    cent = R.unit_rows(rng, 16, dim)
    clustered = cent[rng.integers(0, 16, n)] + 0.3 * rng.standard_normal((n, dim)).astype(np.float32) / np.sqrt(dim)
    yield "clusters", clustered.astype(np.float32)
    sparse = base * (rng.random((n, dim)) < 0.1)
    yield "sparse rows", sparse.astype(np.float32)
    one = np.zeros((n, dim), np.float32)
    one[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], n)
    one[::3] = base[::3]
    yield "one-hot and dense rows mixed", one
    yield "six decades", R.six_decades(rng, n, dim)


def hostile_queries(rng, rows, dim):
    """tests/test_gpu_int8_filter.py::hostile_queries."""
    nq = 24
    q = rows[rng.integers(0, rows.shape[0], nq)] + (0.2 * rng.standard_normal((nq, dim))).astype(np.float32)
    q[1] *= 37.5
    q[2] *= 1e-6
    q[3] = 0.0
    q[3, 7] = 1.0
    q[4] = np.sign(q[4]) * 0.25
    q[5] = np.sign(q[5]) * ((rng.integers(0, 126, dim) + 0.5) / 127.0).astype(np.float32)
    q[5, 0] = 1.0
    q[6, :] = 0.003
    q[6, 0] = 1.0
    q[7] = rng.standard_normal(dim).astype(np.float32) * 900.0
    return q.astype(np.float32)


def reference_scores(oracle, rows, q, hreduce):
    """dot_product_f32_bytes_f32 of every row (the oracle's exhaustive search with k = n, scattered back by row)."""
    n = rows.shape[0]
    r, s = oracle.search_top_k_f32(rows, q, n, hreduce=hreduce)
    assert len(r) == n
    out = np.empty(n, np.float32)
    out[r] = s
    return out


@pytest.mark.parametrize("dim", [128, 384])
def test_bound_covers_every_f32_row_against_float64_and_the_reference_order(oracle, dim):
    rng = np.random.default_rng(5000 + dim)
    worst = 0.0
    for name, rows in corpora(rng, N, dim):
        rows = np.ascontiguousarray(rows, dtype=np.float32)
        stats, r8 = R.slab_stats(rows)
        assert stats[4], name
        q = hostile_queries(rng, rows, dim)
        bounds = [R.query_bound(q[i], stats, dim) for i in range(q.shape[0])]
        delta = np.array([b[0] for b in bounds], np.float64)
        c_q = np.array([float(b[1]) for b in bounds], np.float64)
        p = np.stack([b[2] for b in bounds]).astype(np.int8)
        assert np.all(delta > 0), (name, delta)
        idot = R.int_scores(r8, p)                                                          # [n, nq], exact
        assert np.array_equal(idot[:50], r8[:50].astype(np.int64) @ p.astype(np.int64).T)   # (the f32 product IS exact)
        unit = float(stats[0]) * c_q
        s64 = rows.astype(np.float64) @ q.astype(np.float64).T
        err64 = np.abs(idot - s64 * unit[None, :])
        assert np.all(err64 <= delta[None, :]), (name, float((err64 / delta[None, :]).max()))
        for i in range(q.shape[0]):
            for mode in (0, 1, 2):
                s = reference_scores(oracle, rows, q[i], mode).astype(np.float64)
                assert np.all(np.abs(idot[:, i] - s * unit[i]) <= delta[i]), (name, i, mode)
        worst = max(worst, float((err64 / delta[None, :]).max()))
    assert worst > 0.05, worst   # not vacuous: somewhere the error comes within a factor 20 of the bound


def test_uncertifiable_slabs_are_marked():
    rng = np.random.default_rng(3)
    rows = R.unit_rows(rng, 500, 64)
    q = rows[0]
    for poison in (1e6, np.nan, np.inf, -np.inf):
        bad = rows.copy()
        bad[123, 17] = poison
        stats, _ = R.slab_stats(bad)
        assert not stats[4] and R.query_bound(q, stats, 64)[0] < 0, poison
    stats, r8 = R.slab_stats(np.zeros((10, 64), np.float32))
    assert not stats[4] and not r8.any()
    stats, _ = R.slab_stats(rows * np.float32(65504.0 / np.abs(rows).max()))   # the edge itself is certifiable
    assert stats[4]
    # quant_i8: half away from zero, clamp, NaN -> 0
    got = R.quantize_rows_i8(np.array([[0.5, -0.5, 1.5, -2.5, 0.49999997, 200.0, -200.0, np.nan]], np.float32), 1.0)
    assert got.tolist() == [[1, -1, 2, -3, 0, 127, -127, 0]]


@pytest.mark.parametrize("dim,n", R.SHAPES)
def test_rows_within_the_margin_of_the_kth_best_fit_the_candidate_pool(dim, n, capsys):
    """Per case of the GPU test: the largest count over queries of rows with idot >= a_k - 2 delta (a_k = the k-th best integer
    score among live, allowed rows) — printed, and held to kSelectPool = 1,024."""
    rows, cent = R.clustered_case(dim, n)
    stats, r8 = R.slab_stats(rows)
    assert stats[4]
    import torch   # (multi-threaded GEMM / top-k / counts: numpy's partition alone took a minute over these shapes)
    r8t = torch.from_numpy(r8.astype(np.float32)).T.contiguous()                        # [dim, rows]
    worst = {}
    live_sets = (("all", None), ("60% live", R.case_live(dim, n))) if dim != 384 else (("all", None),)
    neg = torch.tensor(-np.inf, dtype=torch.float32)
    for nq, k in R.CASES:
        q = R.case_queries(dim, n, nq, k, rows, cent)
        bounds = [R.query_bound(q[i], stats, dim) for i in range(nq)]
        delta = np.array([b[0] for b in bounds], np.float64)
        assert np.all(delta > 0)
        p = torch.from_numpy(np.stack([b[2] for b in bounds]).astype(np.float32))
        for q0 in range(0, nq, 256):
            idot = p[q0:q0 + 256] @ r8t                                                   # [queries, rows]: exact integers in f32
            two_delta = torch.from_numpy(2.0 * delta[q0:q0 + 256])[:, None]
            for label, live in live_sets:
                masks = [(label, live)]
                if label == "all" and (nq, k) == (255, 30):
                    masks.append(("allow", R.case_allow(dim, n)))
                for mlabel, mask in masks:
                    sc = idot if mask is None else torch.where(torch.from_numpy(mask)[None, :], idot, neg)
                    ak = sc.topk(k, dim=1).values[:, k - 1:k].double()                   # k-th best per query (live, allowed rows)
                    count = (sc.double() >= ak - two_delta).sum(dim=1)
                    key = (nq, k, mlabel)
                    worst[key] = max(worst.get(key, 0), int(count.max()))
    with capsys.disabled():
        for key, c in worst.items():
            print(f"\n[f32 filter contract] dim {dim} rows {n}: nq {key[0]} k {key[1]} ({key[2]}): at most {c} rows within 2 delta of the k-th best", end="")
    assert max(worst.values()) <= 1024, worst

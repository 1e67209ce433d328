"""numpy restatement of what the device builds for the int8 filter of a Quantization::F32 slab (test infrastructure).

An F32 index filters its batches on an int8 copy of its f32 rows (vector_index_batched.cpp, ensure_filter_copy; the kernels are
int8_kernels.hip's maxabs_f32_kernel / quantize_f32_i8_kernel / i8_stats_f32_kernel) and re-scores the candidates from the f32
rows in dot_product_f32_bytes_f32's order (simd.rs:581-702).  The certificate is the one oracle/filter_bound.py restates for F16
slabs — its query half (query_bound) is imported from there —; the slab half, over f32 rows that were never rounded to f16, lives here:

    c_s            fl32(127 / max|x|)                                        (NaN ignored, as fmaxf does)
    r              quant_i8(x, c_s): round half away from zero of fl32(x c_s), clamp to +-127, NaN -> 0
    E2, R1, R2     max over rows of |eps|_2 (|eps_i| = |fl32(x_i c_s) - r_i| + 8e-6), |r|_1, |r|_2
    certifiable    every element finite and max|x| <= 65,504 (prepare_queries_i8_filter_kernel's slab_bad otherwise)

Unrotated copies only: the rotated copy's matrix comes from libm calls whose last bits need not agree between a host compiler and
numpy; tests/test_gpu_f32_batched.py checks the rotated certificate against float64 arithmetic instead.

Also here: the corpora and queries the CPU contract test and the GPU tests share, so that what the CPU test says about a GPU
case (how many rows sit inside the margin of the k-th best) is said about the very same numbers.
"""
from __future__ import annotations

import numpy as np

from oracle import filter_bound as fb

F32 = np.float32


def quantize_rows_i8(rows_f32: np.ndarray, c_s) -> np.ndarray:
    """quant_i8 (int8_kernels.hip) over f32 rows: round half away from zero, clamp, NaN -> 0."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = (np.ascontiguousarray(rows_f32, dtype=F32) * F32(c_s)).astype(F32)
        r = np.sign(v).astype(np.float64) * np.floor(np.abs(v).astype(np.float64) + 0.5)   # (f64: |v| + 0.5 is exact there)
        r = np.where(np.isnan(r), 0.0, np.clip(r, -127.0, 127.0))
    return r.astype(np.int8)


def slab_scale(rows_f32: np.ndarray):
    """c_s = fl32(127 / max|x|), 0 for a slab of zeros (or of nothing but NaN)."""
    x = np.ascontiguousarray(rows_f32, dtype=F32)
    with np.errstate(invalid="ignore"):
        m = np.abs(x)
        max_abs = F32(np.nanmax(m)) if x.size and not np.all(np.isnan(m)) else F32(0)
    if not (max_abs > 0):
        return F32(0), max_abs
    with np.errstate(over="ignore"):
        return F32(127.0) / max_abs, max_abs


def slab_stats(rows_f32: np.ndarray):
    """(c_s, E2, R1, R2, certifiable) in the layout oracle.filter_bound.query_bound takes, + the int8 rows."""
    x = np.ascontiguousarray(rows_f32, dtype=F32)
    c_s, max_abs = slab_scale(x)
    with np.errstate(invalid="ignore"):
        ok = bool(x.size) and bool(np.all(np.abs(x) <= 65504.0)) and bool(max_abs > 0)
    r8 = quantize_rows_i8(x, c_s) if max_abs > 0 else np.zeros(x.shape, np.int8)
    if not ok:
        return (c_s, 0.0, 0.0, 0.0, False), r8
    # (row sums in f64 / int64 over f32 / int32 elements: exact enough for maxima that the kernel itself accumulates in f32)
    eps = np.abs((x * c_s).astype(F32) - r8.astype(F32)) + F32(8e-6)
    e2 = float(np.sqrt(np.einsum("ij,ij->i", eps, eps, dtype=np.float64).max())) * 1.001
    r = r8.astype(np.int32)
    r1 = float(np.abs(r).sum(axis=1, dtype=np.int64).max())
    r2 = float(np.sqrt(np.einsum("ij,ij->i", r, r, dtype=np.int64).max()))
    return (c_s, e2, r1, r2, True), r8


def query_bound(q: np.ndarray, stats, dim: int):
    """(delta, c_q, p) exactly as prepare_queries_i8_filter_kernel computes them (oracle/filter_bound.py's restatement: the
    kernel never sees the slab's element type)."""
    return fb.query_bound(q, stats, dim)


def int_scores(rows_i8: np.ndarray, queries_i8: np.ndarray) -> np.ndarray:
    """[n, nq] exact integer scores (|sum| <= 127^2 x dim < 2^24 for dim <= 1040: exact in f32, so BLAS may do it)."""
    assert rows_i8.shape[1] <= 1040
    return (rows_i8.astype(F32) @ queries_i8.astype(F32).T).astype(np.int64)


# ---- shared corpora -----------------------------------------------------------------------------------------------------------

def unit_rows(rng, n, dim):
    x = rng.standard_normal((n, dim)).astype(F32)
    return x / np.linalg.norm(x, axis=1, keepdims=True)


def six_decades(rng, n, dim):
    """Elements spread over six decades inside +-65,504: per row in the first half, per ELEMENT in the second — where the order of
    a row's additions decides the last bits of its score."""
    base = unit_rows(rng, n, dim)
    scale = np.empty((n, dim), F32)
    scale[: n // 2] = (10.0 ** rng.uniform(-2.0, 4.0, (n // 2, 1))).astype(F32)
    scale[n // 2:] = (10.0 ** rng.uniform(-2.0, 4.0, (n - n // 2, dim))).astype(F32)
    out = (base * scale).astype(F32)
    assert np.abs(out).max() <= 65504.0
    return out


def clustered_case(dim: int, n: int):
    """The clustered corpus of test_gpu_int8_filter.py::test_group_maxima_sample_stage..., kept as f32: (rows, centroids).  Rows
    70,000-70,039 repeat row 69,999 when the corpus has them; the ragged tail holds near-duplicates of row 123."""
    rng = np.random.default_rng(9000 + dim * 7 + n % 1000)
    cent = unit_rows(rng, 32, dim)
    rows = cent[rng.integers(0, 32, n)] + 0.3 * rng.uniform(-1, 1, (n, dim)).astype(F32)
    rows /= np.linalg.norm(rows, axis=1, keepdims=True)
    if n > 70_040:
        rows[70_000:70_040] = rows[69_999]
    tail = n % 64 if n % 64 else 19
    rows[n - tail:] = rows[123] + 1e-3 * rng.standard_normal((tail, dim)).astype(F32)
    return np.ascontiguousarray(rows, dtype=F32), cent


CASES = ((17, 10), (128, 64), (129, 10), (255, 30), (384, 1), (640, 24), (1030, 10))
SHAPES = ((64, 33_001), (128, 33_001), (256, 200_003), (256, 262_163), (384, 262_163))


def case_queries(dim: int, n: int, nq: int, k: int, rows: np.ndarray, cent: np.ndarray):
    rng = np.random.default_rng(77_000 + dim + n % 997 + nq * 13 + k)
    q = cent[rng.integers(0, 32, nq)] + 0.3 * rng.uniform(-1, 1, (nq, dim)).astype(F32)
    q[0] = rows[123]
    if n > 70_040:
        q[1] = rows[69_999]
    return np.ascontiguousarray(q, dtype=F32)


def case_live(dim: int, n: int):
    return np.random.default_rng(31_000 + dim + n % 991).random(n) < 0.6


def case_allow(dim: int, n: int):
    return np.random.default_rng(32_000 + dim + n % 983).random(n) < 0.5

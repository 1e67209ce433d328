"""CPU checks of the query-hubness correction: the reference's inline tests with their literals (hubness.rs:175-362,
searcher.rs:6583-6613, types.rs cmp_rank), the host restatement in libfsgpu.so (fsgpu_query_hubness, fsgpu_apply_hubness_penalty)
against tests/hubness_ref.py bit for bit, the derived bound that links the pinned sum order to every order the reference can
produce, the kernel's ISA, and the error paths that need no device."""
import ctypes as C
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hubness_ref as H  # noqa: E402

F32 = np.float32


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same_values(a, b):
    """equal bits; NaNs compare as NaN; zeros by value"""
    a, b = np.asarray(a, F32), np.asarray(b, F32)
    return a.shape == b.shape and bool(np.all((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b)) | ((a == 0) & (b == 0))))


def hit(index, score):
    return (f"d{index}", score, index)


# ---- the restatement's own dot against the oracle ----

@pytest.mark.parametrize("dim", [2, 43, 100, 256, 384])
def test_ref_dot_equals_the_oracle_bit_for_bit(oracle, dim):
    rng = np.random.default_rng(dim)
    x = (rng.standard_normal((20, dim)) * np.exp(rng.uniform(-3, 3, (20, 1)))).astype(F32)
    y = rng.standard_normal((15, dim)).astype(F32)
    for mode in (H.HREDUCE_SSE2, H.HREDUCE_AVX, H.HREDUCE_SEQ):
        got = H.dot_many(x, y, mode)
        want = np.array([[oracle.dot_f32_f32(x[i], y[j], mode) for j in range(15)] for i in range(20)], dtype=F32)
        assert np.array_equal(bits(got), bits(want)), (dim, mode)   # 300 pairs per dimension and order


# ---- hubness.rs inline tests, with their literals ----

def test_beta_zero_is_identity():
    fa = _fa()
    hits = [hit(0, 0.9), hit(1, 0.5)]
    out = fa.apply_hubness_penalty(hits, [0.8, 0.3], fa.HubnessConfig(beta=0.0, kq=10))
    assert [(d, i) for d, _, i in out] == [(d, i) for d, _, i in hits]
    assert np.array_equal(bits([s for _, s, _ in out]), bits([0.9, 0.5]))
    for beta in (-1.0, float("nan"), float("inf")):
        out = fa.apply_hubness_penalty(hits, [0.8, 0.3], fa.HubnessConfig(beta=beta))
        assert np.array_equal(bits([s for _, s, _ in out]), bits([0.9, 0.5]))
    assert fa.HubnessConfig().beta == pytest.approx(0.2) and fa.HubnessConfig().kq == 10
    from frankensearch_amd.hubness import _HubnessConfig
    c = _HubnessConfig()
    assert fa._lib.lib().fsgpu_hubness_config_default(C.addressof(c)) == 0
    assert c.beta == F32(0.2) and c.kq == 10 and list(c.reserved) == [0, 0, 0, 0]


def test_penalty_subtracts_beta_times_hubness_by_index():
    fa = _fa()
    out = fa.apply_hubness_penalty([hit(0, 0.3), hit(1, 0.9)], [0.1, 0.8], fa.HubnessConfig(beta=0.5), resort=False)
    assert abs(out[0][1] - (0.3 - 0.05)) < 1e-6
    assert abs(out[1][1] - (0.9 - 0.40)) < 1e-6
    # a separate f32 multiply and subtract
    want = H.apply_hubness_penalty([hit(0, 0.3), hit(1, 0.9)], [0.1, 0.8], 0.5, resort=False)
    assert np.array_equal(bits([s for _, s, _ in out]), bits([s for _, s, _ in want]))


def test_out_of_range_index_gets_no_penalty():
    fa = _fa()
    out = fa.apply_hubness_penalty([hit(7, 0.6)], [0.9, 0.9], fa.HubnessConfig(beta=0.5))
    assert abs(out[0][1] - 0.6) < 1e-6


def test_hub_doc_scores_higher_r_d_than_outlier():
    fa = _fa()
    r = fa.compute_query_hubness([[1.0, 0.0], [0.0, 1.0]], [[1.0, 0.0], [1.0, 0.0]], 10)
    assert abs(r[0] - 1.0) < 1e-6 and abs(r[1]) < 1e-6


def test_hubness_averages_kq_nearest_queries():
    fa = _fa()
    r = fa.compute_query_hubness([[1.0, 0.0]], [[1.0, 0.0], [0.6, 0.8], [0.0, 1.0]], 2)
    assert abs(r[0] - 0.8) < 1e-6


def test_hubness_matches_scalar_reference_across_kernel_blocks():
    fa = _fa()
    dim = 43   # one group of 32 + one leftover chunk + a tail of 3

    def mk(seed):
        raw = np.array([np.sin(F32(i) * F32(seed)) for i in range(dim)], dtype=F32)
        return (raw / np.sqrt(np.sum(raw * raw, dtype=F32))).astype(F32)

    docs, queries = [mk(0.7), mk(1.3)], [mk(2.1), mk(0.35)]
    r = fa.compute_query_hubness(docs, queries, 2)
    for i, d in enumerate(docs):
        expect = F32(0)
        for q in queries:
            s = F32(0)
            for x, y in zip(d, q):
                s = F32(s + F32(x * y))
            expect = F32(expect + s)
        assert abs(r[i] - expect / F32(2)) < 1e-6


def test_ragged_lengths_truncate_to_common_prefix():
    fa = _fa()
    r = fa.compute_query_hubness([[1.0, 0.0, 0.0]], [[1.0, 0.0]], 1)
    assert abs(r[0] - 1.0) < 1e-6
    rng = np.random.default_rng(5)
    docs = [rng.standard_normal(n).astype(F32) for n in (50, 43, 8, 100, 1)]
    queries = [rng.standard_normal(n).astype(F32) for n in (43, 64, 7, 100)]
    assert same_values(fa.compute_query_hubness(docs, queries, 3), H.compute_query_hubness_ragged(docs, queries, 3))


def test_empty_sample_is_zero_hubness():
    fa = _fa()
    assert fa.compute_query_hubness([[1.0, 0.0]], [], 10).tolist() == [0.0]
    assert fa.compute_query_hubness([[1.0, 0.0], [0.5, 0.5]], [[1.0, 0.0]], 0).tolist() == [0.0, 0.0]
    assert fa.compute_query_hubness([], [[1.0, 0.0]], 3).size == 0


def test_demotes_a_hub_below_a_specific_relevant():
    fa = _fa()
    out = fa.apply_hubness_penalty([hit(0, 0.80), hit(1, 0.72)], [0.75, 0.20], fa.HubnessConfig(beta=0.3), resort=False)
    assert out[1][1] > out[0][1]
    out = fa.apply_hubness_penalty([hit(0, 0.80), hit(1, 0.72)], [0.75, 0.20], fa.HubnessConfig(beta=0.3))
    assert [d for d, _, _ in out] == ["d1", "d0"]


# ---- searcher.rs:6583-6613 and the cmp_rank cases ----

def test_hub_drops_below_an_equal_scoring_peer_and_the_pool_is_resorted():
    fa = _fa()
    hits = [("doc-4", 1.0, 4), ("doc-0", 1.0, 0), ("doc-1", 0.2, 1)]
    out = fa.apply_hubness_penalty(hits, [0.0, 0.0, 0.0, 0.0, 1.0], fa.HubnessConfig(beta=0.5))
    assert [d for d, _, _ in out] == ["doc-0", "doc-4", "doc-1"]
    assert abs(out[1][1] - 0.5) < 1e-6 and abs(out[0][1] - 1.0) < 1e-6
    assert [i for _, _, i in out] == [0, 4, 1]


def test_cmp_rank_breaks_ties_by_doc_id_and_sorts_nan_last():
    fa = _fa()
    table = [0.0] * 8
    cfg = fa.HubnessConfig(beta=0.5)
    out = fa.apply_hubness_penalty([("b", 0.5, 0), ("a", 0.5, 1), ("c", 0.5, 2), ("aa", 0.5, 3)], table, cfg)
    assert [d for d, _, _ in out] == ["a", "aa", "b", "c"]
    nan, inf = float("nan"), float("inf")
    hits = [("n", nan, 0), ("lo", -inf, 1), ("hi", inf, 2), ("z", 0.0, 3), ("mz", -0.0, 4), ("m", nan, 5), ("x", 0.25, 6)]
    out = fa.apply_hubness_penalty(hits, table, cfg)
    # NaN ranks as -inf: after every real value, tied with -inf, doc id ascending among them; -0.0 below +0.0
    assert [d for d, _, _ in out] == ["hi", "x", "z", "mz", "lo", "m", "n"]
    want = H.apply_hubness_penalty(hits, table, 0.5)
    assert [d for d, _, _ in out] == [d for d, _, _ in want]
    rng = np.random.default_rng(3)
    for _ in range(20):
        n = int(rng.integers(1, 40))
        hits = [(f"doc-{int(rng.integers(0, 15))}", float(rng.choice([0.1, 0.5, 0.5, 0.9, nan, -0.0, 0.0])), int(rng.integers(0, 12))) for _ in range(n)]
        tab = rng.random(10).astype(F32)
        got = fa.apply_hubness_penalty(hits, tab, fa.HubnessConfig(beta=0.37))
        want = H.apply_hubness_penalty(hits, tab, 0.37)
        assert [(d, i) for d, _, i in got] == [(d, i) for d, _, i in want]
        assert same_values([s for _, s, _ in got], [s for _, s, _ in want])
    from frankensearch_amd.hubness import _HubnessConfig
    from frankensearch_amd.fusion import _pack
    bad = _HubnessConfig(0.5, 10)
    bad.reserved[2] = 1
    arr, keep = _pack([("a", 1.0, 0)])
    assert fa._lib.lib().fsgpu_apply_hubness_penalty(arr, 1, None, 0, C.addressof(bad), 1, None) == fa._lib.ERR_INVALID_CONFIG


# ---- fsgpu_query_hubness == the numpy restatement, bit for bit ----

@pytest.mark.parametrize("dim", [4, 43, 100, 256, 384, 768])
def test_host_restatement_equals_the_numpy_restatement_bit_for_bit(dim):
    fa = _fa()
    rng = np.random.default_rng(100 + dim)
    docs, queries = H.unit_rows(rng, 90, dim), H.unit_rows(rng, 70, dim)
    docs[7, dim // 2] = np.inf          # one row holding an inf
    queries[11, :] = np.nan             # one NaN query
    for mode in (H.HREDUCE_SSE2, H.HREDUCE_AVX, H.HREDUCE_SEQ):
        for kq in (1, 2, 10, 64, 100):  # 100 > Q = 70: k clamps to the sample
            got = fa.compute_query_hubness(docs, queries, kq, hreduce=mode)
            want = H.compute_query_hubness(docs, queries, kq, mode)
            assert same_values(got, want), (dim, mode, kq, np.flatnonzero(bits(got) != bits(want))[:5])
    # the NaN query is a +NaN similarity for every row: it sorts above +inf and poisons every mean, as in the reference
    assert np.all(np.isnan(fa.compute_query_hubness(docs, queries, 3)))
    clean = np.delete(queries, 11, axis=0)
    got = fa.compute_query_hubness(docs, clean, 10)
    assert np.isfinite(np.delete(got, 7)).all() and not np.isfinite(got[7])


def test_a_rows_value_does_not_depend_on_its_neighbours_or_on_the_thread_count():
    """hubness_par_matches_serial_across_threshold (hubness.rs:275-327): 2 x 60 dots run serially, 200 x 60 on the thread pool."""
    fa = _fa()
    dim = 32

    def mk(seed):
        raw = np.array([np.cos(F32(i) * F32(seed) + F32(seed)) for i in range(dim)], dtype=F32)
        return (raw / np.sqrt(np.sum(raw * raw, dtype=F32))).astype(F32)

    queries = [mk(0.11 * (i + 1)) for i in range(60)]
    d0, d1, filler = mk(3.7), mk(9.1), mk(1.9)
    serial = fa.compute_query_hubness([d0, d1], queries, 10)
    saved = os.environ.get("OMP_NUM_THREADS")
    try:
        for threads in ("1", "16"):
            os.environ["OMP_NUM_THREADS"] = threads
            par = fa.compute_query_hubness([d0, d1] + [filler] * 198, queries, 10)
            assert par.size == 200
            assert np.array_equal(bits(par[:2]), bits(serial))
            assert np.all(bits(par[2:]) == bits(par[2]))
    finally:
        if saved is None:
            os.environ.pop("OMP_NUM_THREADS", None)
        else:
            os.environ["OMP_NUM_THREADS"] = saved
    assert np.array_equal(bits(serial), bits(H.compute_query_hubness(np.stack([d0, d1]), np.stack(queries), 10)))


def test_canonical_order_and_every_permutation_obey_the_derived_bound():
    """The reference sums `top` in an unspecified order (hubness.rs:135-137).  With R_d the f64 mean of the k selected f32 sims,
    every order of k - 1 adds and one division, each rounding once, obeys |r_d - R_d| <= gamma_k * mean|v_i| with
    gamma_k = k u / (1 - k u), u = 2^-24.  So does the reference's result, whatever order its select left."""
    fa = _fa()
    rng = np.random.default_rng(77)
    k, n = 10, 400
    docs, queries = H.unit_rows(rng, n, 384), H.unit_rows(rng, 300, 384)
    _, top = H.compute_query_hubness(docs, queries, k, want_topk=True)
    got = fa.compute_query_hubness(docs, queries, k)
    u = 2.0 ** -24
    gamma = k * u / (1 - k * u)
    exact = top.astype(np.float64).mean(axis=1)
    bound = gamma * np.abs(top.astype(np.float64)).mean(axis=1)
    err = np.abs(got.astype(np.float64) - exact)
    print(f"canonical order: worst |r_d - R_d| / bound = {float(np.max(err / bound)):.3f} over {n} rows")
    assert np.all(err <= bound)
    sensitive = 0
    for r in range(n):
        seen = {int(bits(got[r:r + 1])[0])}
        for _ in range(6):
            perm = rng.permutation(k)
            pivot, rest = top[r, perm[0]], top[r, perm[1:]]
            s = F32(-0.0)                      # Rust's float Sum starts from -0.0
            for v in rest:
                s = F32(s + v)
            val = F32(F32(pivot + s) / F32(k))
            assert abs(float(val) - exact[r]) <= bound[r], (r, perm)
            seen.add(int(bits(np.asarray([val]))[0]))
        sensitive += len(seen) > 1
    print(f"order-sensitive rows: {sensitive} of {n}")
    assert sensitive >= n // 4, "the sum order would not matter: nothing to pin"


# ---- the kernel's ISA ----

def test_hubness_kernel_has_no_fused_multiply_add():
    """The table build must issue separate multiplies and adds (simd.rs:134-222): the dim-384 and dim-256 instantiations hold packed
    or scalar f32 mul / add and none of the fused forms (literal-operand and mixed-precision fmas included), no dot2, no MFMA; the
    runtime-dimension instantiations, whose leftover chunks and tail must be unfused too, are held to the same."""
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build

    build()
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    if not os.path.exists(objdump):
        pytest.skip("llvm-objdump not available")
    obj = os.path.join(os.path.dirname(_lib.LIB_PATH), "_build", "hubness_kernels.o")
    tmp = tempfile.mkdtemp(prefix="fsgpu_isa_")
    shutil.copy(obj, os.path.join(tmp, "hubness_kernels.o"))
    subprocess.check_call([objdump, "--offloading", "hubness_kernels.o"], cwd=tmp, stdout=subprocess.DEVNULL)
    outs = glob.glob(os.path.join(tmp, "*gfx950*"))
    assert outs, "no gfx950 code object in hubness_kernels.o"
    asm = subprocess.check_output([objdump, "-d", outs[0]]).decode()
    seen = 0
    fused = r"v_(pk_)?fma_f32|v_fmaak_f32|v_fmamk_f32|v_fma_mix|v_fmac_f32|v_mac_f32|v_mad_f32|v_dot2|v_mfma|v_smfma"
    for b in re.split(r"\n(?=[0-9a-f]+ <)", asm):
        head = b.split("\n", 1)[0]
        # <384, *> and <256, *>, and the runtime-dimension <0, *> whose leftover chunks and tail are unfused too
        if "hubness_kernelILi384E" in head or "hubness_kernelILi256E" in head or "hubness_kernelILi0E" in head:
            seen += 1
            assert re.search(r"v_pk_mul_f32|v_mul_f32", b) and re.search(r"v_pk_add_f32|v_add_f32", b), head
            assert not re.search(fused, b), head
            assert "scratch_" not in b, head
    assert seen >= 9   # three dimensions x three horizontal orders


# ---- errors that need no device ----

def test_no_device_and_null_arguments():
    import torch
    fa = _fa()
    L = fa._lib.lib()
    q = np.zeros((2, 8), F32)
    out = np.zeros(4, F32)
    if not torch.cuda.is_available():
        assert L.fsgpu_index_compute_query_hubness(None, q.ctypes.data, 2, 8, 10, out.ctypes.data) == fa._lib.ERR_NO_DEVICE
        assert L.fsgpu_sharded_compute_query_hubness(None, q.ctypes.data, 2, 8, 10, out.ctypes.data) == fa._lib.ERR_NO_DEVICE
        assert "no HIP device" in fa._lib.last_error()
    else:
        assert L.fsgpu_index_compute_query_hubness(None, q.ctypes.data, 2, 8, 10, out.ctypes.data) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_query_hubness(None, None, 2, None, None, 0, 3, 0, None) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_query_hubness(None, None, 0, None, None, 0, 3, 7, None) == fa._lib.ERR_INVALID_CONFIG
    assert L.fsgpu_hubness_config_default(None) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_apply_hubness_penalty(None, 3, None, 0, None, 1, None) == fa._lib.ERR_NULL_ARGUMENT
    from frankensearch_amd import host
    assert "fshost_two_tier_set_hubness" in host.SYMBOLS
    assert host.lib().fshost_two_tier_set_hubness(None, None, 0, 0.5) == fa._lib.ERR_NULL_ARGUMENT

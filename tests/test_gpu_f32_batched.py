"""Batched search on Quantization::F32 slabs through the int8 matrix-core filter.

An F32 index (raw little-endian f32 rows, dot_product_f32_bytes_f32: simd.rs:581-702) filters its batches on an int8 copy of its
rows and re-scores the candidates from the f32 rows in the reference's operation order, inside the selections (mfma_scan.hip:
select_kernel / select_groups_kernel with F32 rows).  The contract is the one every batched path has: rows, score bits and counts
equal the exact kernels' (search_batch(exact=True)) and oracle.search_top_k_f32, in any batch and every reduce_add order — and
the PATH is the matrix-core one: the int8 filter counts the queries, the main pass is a scan_wide / scan_mfma instantiation, and
few queries fall back.  Corpora and queries of the first test come from tests/f32_filter_ref.py, whose CPU test counts, for
the same numbers, the rows within the margin of the k-th best (a necessary condition for the fallback cap below to hold).
"""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import f32_filter_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
_cache = {}   # corpora: computed once, never changed


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    assert fa_mod._lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    return fa_mod


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def corpus(dim, n):
    if (dim, n) not in _cache:
        _cache[(dim, n)] = R.clustered_case(dim, n)
    return _cache[(dim, n)]


def main_pass_kernel(fa):
    return fa._lib.lib().fsgpu_last_main_pass_kernel().decode()


def exact_in_slices(idx, q, k, allow=None):
    parts = [idx.search_batch(q[s:s + 64], k, allow=allow, exact=True) for s in range(0, q.shape[0], 64)]
    return tuple(np.concatenate([p[i] for p in parts]) for i in range(3))


def assert_same(got, want, what):
    br, bs, bc = got[:3]
    er, es, ec = want
    assert np.array_equal(bc, ec) and np.array_equal(br, er) and np.array_equal(bits(bs), bits(es)), what


def assert_oracle(oracle, rows, q, k, got_rows, got_scores, live=None, hreduce=0, what=None):
    orow, osc = oracle.search_top_k_f32(rows, q, k, live=live, hreduce=hreduce)
    assert np.array_equal(got_rows[:len(orow)], orow) and np.array_equal(bits(got_scores[:len(osc)]), bits(osc)), what


# ---- 1. the matrix path runs and gives the exact bits ---------------------------------------------------------------------------

@pytest.mark.parametrize("dim,n", R.SHAPES)
def test_f32_batches_take_the_int8_matrix_path_and_give_the_exact_bits(fa, oracle, dim, n):
    """33,001 rows (ragged last tile) reach the LDS-query kernel at dims 64 / 128; 200,003 and 262,163 rows reach the
    register-resident-query main pass and its group-maxima sample at dims 256 / 384 from 129 queries on.  (A 1,030-query batch is a
    1,024-query round and a 6-query tail, whose main pass is the LDS-query kernel whatever the dimension: the kernel name is held
    to the LAST round's size, and the 1,024-query round is searched once more on its own to see the wide kernel's name.)"""
    rows, cent = corpus(dim, n)
    tail = n % 64 if n % 64 else 19
    wide_dim = dim in (256, 384)
    for live in ((None, R.case_live(dim, n)) if dim != 384 else (None,)):
        idx = fa.VectorIndex.from_slab_f32(rows, live=live)
        for nq, k in R.CASES:
            q = R.case_queries(dim, n, nq, k, rows, cent)
            allow = R.case_allow(dim, n) if (nq, k) == (255, 30) and live is None else None
            eff = allow if live is None else live
            want = exact_in_slices(idx, q, k, allow)
            for rep in range(2):
                before = idx.batched_filter_stats()["int8_queries"]
                br, bs, bc, fb = idx.search_batched(q, k, allow=allow)
                what = (dim, n, nq, k, live is not None, allow is not None, rep)
                assert_same((br, bs, bc), want, what)
                assert idx.batched_filter_stats()["int8_queries"] - before == nq, what
                last_round = nq % 1024 or 1024
                name = main_pass_kernel(fa)
                assert ("scan_wide_kernel" if wide_dim and last_round >= 129 else "scan_mfma_kernel") in name, (what, name)
                assert fb <= nq // 8, (what, fb)
            if wide_dim and nq > 1024:
                br2, bs2, bc2, fb2 = idx.search_batched(q[:1024], k)
                assert_same((br2, bs2, bc2), tuple(w[:1024] for w in want), (dim, n, "first round alone"))
                assert "scan_wide_kernel" in main_pass_kernel(fa) and fb2 <= 128
            assert_oracle(oracle, rows, q[0], k, br[0], bs[0], live=eff, what=(dim, n, nq, k, "probe"))
            # the ragged tail holds near-copies of the probe's row: they are among its best hits
            tail_rows = np.arange(n - tail, n)
            tail_ok = tail_rows if eff is None else tail_rows[eff[tail_rows]]
            # (row 123 itself may take one of the k places)
            assert np.isin(tail_ok, br[0][:bc[0]]).sum() >= min(k - 1, len(tail_ok)), (dim, n, nq, k)
            if n > 70_040:   # identical rows 69,999 .. 70,039 (score 1 against query 1): the lower row wins
                ident = np.arange(69_999, 70_040)
                ident = ident if eff is None else ident[eff[ident]]
                m = min(k, len(ident))
                assert np.array_equal(br[1][:m], ident[:m].astype(np.uint32)), (dim, n, nq, k, br[1][:m])
        assert idx.batched_filter_stats()["int8_active"]
        idx.close()


# ---- 2. the certificate against float64 and the exact kernels -------------------------------------------------------------------

def gpu_corpora(rng, n, dim):
    """tests/test_gpu_int8_filter.py::corpora kept as f32 + the six-decade corpus."""
    base = R.unit_rows(rng, n, dim)
    yield "gaussian unit rows", base
    out = base.copy()
    out[:, rng.integers(0, dim, 3)] *= 12.0
    yield "outlier dimensions", (out / np.linalg.norm(out, axis=1, keepdims=True)).astype(F32)
    yield "tiny magnitudes", base * F32(3e-3)
    yield "large magnitudes", base * F32(180.0)
    cent = R.unit_rows(rng, 16, dim)
    yield "clusters", (cent[rng.integers(0, 16, n)] + 0.3 * rng.standard_normal((n, dim)).astype(F32) / np.sqrt(dim)).astype(F32)
    yield "sparse rows", (base * (rng.random((n, dim)) < 0.1)).astype(F32)
    one = np.zeros((n, dim), F32)
    one[np.arange(n), rng.integers(0, dim, n)] = rng.choice([-1.0, 1.0], n)
    one[::3] = base[::3]
    yield "one-hot and dense rows mixed", one
    yield "six decades", R.six_decades(rng, n, dim)


def hostile_queries(rng, rows, dim):
    nq = 24
    q = rows[rng.integers(0, rows.shape[0], nq)] + (0.2 * rng.standard_normal((nq, dim))).astype(F32)
    q[1] *= 37.5
    q[2] *= 1e-6
    q[3] = 0.0
    q[3, 7] = 1.0
    q[4] = np.sign(q[4]) * 0.25
    q[5] = np.sign(q[5]) * ((rng.integers(0, 126, dim) + 0.5) / 127.0).astype(F32)
    q[5, 0] = 1.0
    q[6, :] = 0.003
    q[6, 0] = 1.0
    q[7] = rng.standard_normal(dim).astype(F32) * 900.0
    return q.astype(F32)


@pytest.mark.parametrize("dim", [128, 384])
def test_f32_bound_covers_every_row_against_float64_and_the_exact_kernels(fa, oracle, dim):
    """The F32 twin of test_bound_covers_every_row_against_float64_and_the_exact_kernels: 12,000 rows (below the search gate, but
    what int8_filter_bound serves), unrotated copy; the device's int8 rows and delta equal tests/f32_filter_ref.py's."""
    rng = np.random.default_rng(1000 + dim)
    n = 12_000
    worst = 0.0
    for name, rows in gpu_corpora(rng, n, dim):
        rows = np.ascontiguousarray(rows, dtype=F32)
        idx = fa.VectorIndex.from_slab_f32(rows)
        idx.set_filter_rotation(1)
        q = hostile_queries(rng, rows, dim)
        delta, qscale, sscale, qi8, slab_i8 = idx.int8_filter_bound(q, want_slab=True)
        assert not idx.filter_rotated()
        stats, r8 = R.slab_stats(rows)
        assert np.array_equal(slab_i8, r8), name
        for i in range(q.shape[0]):
            assert np.array_equal(qi8[i], oracle.quantize_query_i8(q[i])), (name, i)
        assert np.all(delta > 0), (name, delta)
        assert abs(float(stats[0]) - sscale) <= 1e-6 * sscale, name
        for i in range(q.shape[0]):
            want = R.query_bound(q[i], stats, dim)[0]
            assert abs(float(delta[i]) - want) <= 2e-3 * want + 2.0, (name, i, float(delta[i]), want)
        idot = R.int_scores(slab_i8, qi8)
        s64 = rows.astype(np.float64) @ q.astype(np.float64).T
        unit = np.float64(sscale) * qscale.astype(np.float64)
        err64 = np.abs(idot - s64 * unit[None, :])
        assert np.all(err64 <= delta[None, :].astype(np.float64)), (name, float((err64 / delta[None, :]).max()))
        for i in (0, 1, 2, 5, 7):
            exact = idx.gather_dot(q[i], np.arange(n, dtype=np.uint32)).astype(np.float64)
            assert np.all(np.abs(idot[:, i] - exact * unit[i]) <= float(delta[i])), (name, i)
        worst = max(worst, float((err64 / delta[None, :]).max()))
        idx.close()
    assert worst > 0.05, worst


# ---- 3. the rotated copy ---------------------------------------------------------------------------------------------------------

def test_f32_rotated_filter_copy_keeps_the_bound_and_the_exact_bits(fa, oracle):
    rng = np.random.default_rng(2256)
    dim, k = 256, 10
    rows = next(r for name, r in gpu_corpora(rng, 70_000, dim) if name == "outlier dimensions")
    rows = np.ascontiguousarray(rows, dtype=F32)
    n = rows.shape[0]
    q = (rows[rng.integers(0, n, 300)] + (0.2 * rng.standard_normal((300, dim)) / np.sqrt(dim)).astype(F32)).astype(F32)
    hq = hostile_queries(rng, rows, dim)
    answers = {}
    for mode in (0, 2, 1):
        idx = fa.VectorIndex.from_slab_f32(rows)
        idx.set_filter_rotation(mode)
        delta, qscale, sscale, qi8, slab_i8 = idx.int8_filter_bound(hq, want_slab=True)
        assert idx.filter_rotated() == (mode != 1), mode
        assert np.all(delta > 0), (mode, delta)
        idot = R.int_scores(slab_i8, qi8)
        s64 = rows.astype(np.float64) @ hq.astype(np.float64).T
        unit = np.float64(sscale) * qscale.astype(np.float64)
        err64 = np.abs(idot - s64 * unit[None, :])
        # (the rotated query scale comes back through an f32 division: 1e-6 relative on S c_s c_q, as in the F16 test)
        slack = 2e-6 * np.abs(s64 * unit[None, :])
        assert np.all(err64 <= delta[None, :].astype(np.float64) + slack), (mode, float((err64 / delta[None, :]).max()))
        want = exact_in_slices(idx, q, k)
        before = idx.batched_filter_stats()["int8_queries"]
        br, bs, bc, fb = idx.search_batched(q, k)
        assert_same((br, bs, bc), want, ("rotation mode", mode))
        assert idx.batched_filter_stats()["int8_queries"] - before == 300 and fb <= 300 // 8, (mode, fb)
        answers[mode] = (br, bs, bc)
        assert_oracle(oracle, rows, q[0], k, br[0], bs[0], what=("rotated", mode))
        if mode == 0:   # margins in score units: the rotation is what narrows them on this corpus
            margin_rot = np.median(delta / (sscale * qscale))
        if mode == 1:
            assert margin_rot < 0.5 * np.median(delta / (sscale * qscale))
        idx.close()
    for mode in (0, 2):
        assert_same(answers[mode], answers[1], ("same answers rotated and not", mode))


# ---- 4. uncertifiable inputs are still answered exactly --------------------------------------------------------------------------

def test_f32_uncertifiable_inputs_are_still_answered_exactly(fa, oracle):
    rng = np.random.default_rng(7)
    n, dim, k = 40_003, 128, 10
    rows = R.unit_rows(rng, n, dim)
    nq = 40
    q = (rows[rng.integers(0, n, nq)] + (0.2 * rng.standard_normal((nq, dim))).astype(F32)).astype(F32)
    q[0] = 0.0
    q[1, 3] = np.nan
    q[2, 5] = np.inf
    q[3, 9] = -np.inf
    q[4, 9] = 70000.0                # |q| > 65,504
    idx = fa.VectorIndex.from_slab_f32(rows)
    delta = idx.int8_filter_bound(q)[0]
    assert np.all(delta[:5] < 0) and np.all(delta[5:] > 0), delta[:8]
    br, bs, bc, fb = idx.search_batched(q, k)
    assert_same((br, bs, bc), exact_in_slices(idx, q, k), "uncertifiable queries")
    st = idx.batched_filter_stats()
    # no f16 filter behind the int8 one: the five go straight to the exact f32 kernels, as fallbacks
    assert st["int8_queries"] == nq and st["refiltered_f16"] == 0 and 5 <= fb <= 8, (st, fb)
    for qi in (0, 4, 17):
        assert_oracle(oracle, rows, q[qi], k, br[qi], bs[qi], what=qi)
    idx.close()
    # a slab with an element of 1e6 has no bound (max |x| > 65,504): every query falls back, with the oracle's bits
    bad = rows.copy()
    bad[12_345, 17] = 1e6
    idx = fa.VectorIndex.from_slab_f32(bad)
    assert np.all(idx.int8_filter_bound(q)[0] < 0)
    br, bs, bc, fb = idx.search_batched(q, k)
    assert fb == nq, fb
    assert_same((br, bs, bc), exact_in_slices(idx, q, k), "slab_bad")
    for qi in (5, 17, 39):
        assert_oracle(oracle, bad, q[qi], k, br[qi], bs[qi], what=("slab_bad", qi))
    idx.close()
    # a NaN row next to the best rows: its neighbours keep their place (a NaN slab has no int8 bound either: exact kernels)
    targets = np.array([4000, 8001, 12_002, 16_003, 20_004, 24_005, 28_006, 32_007])
    tq = (np.tile(rows[targets], (40, 1))[:300] + (0.05 * rng.standard_normal((300, dim))).astype(F32) / np.sqrt(dim)).astype(F32)
    poisoned = rows.copy()
    for t in targets:
        for off in (-2, -1, 1, 2):
            poisoned[t + off, int(rng.integers(0, dim))] = np.nan
    idx = fa.VectorIndex.from_slab_f32(poisoned)
    for nq2 in (70, 300):
        want = exact_in_slices(idx, tq[:nq2], k)
        assert all(int(want[0][i, 0]) == int(targets[i % 8]) for i in range(nq2))
        br, bs, bc, fb = idx.search_batched(tq[:nq2], k)
        assert_same((br, bs, bc), want, ("NaN rows", nq2))
    assert_oracle(oracle, poisoned, tq[3], k, br[3], bs[3], what="NaN rows probe")
    idx.close()
    # six decades inside +-65,504: certifiable, and where a wrong order of a row's additions shows in the score bits
    six = R.six_decades(rng, 40_003, 256)
    sq = (six[rng.integers(0, 40_003, 200)] * (1.0 + 0.1 * rng.standard_normal((200, 256)))).astype(F32)
    idx = fa.VectorIndex.from_slab_f32(six)
    assert np.all(idx.int8_filter_bound(sq[:16])[0] > 0)
    for mode in (0, 1, 2):
        idx.set_hreduce(mode)
        br, bs, bc, fb = idx.search_batched(sq, k)
        assert_same((br, bs, bc), exact_in_slices(idx, sq, k), ("six decades", mode))
        for qi in (0, 77, 199):
            assert_oracle(oracle, six, sq[qi], k, br[qi], bs[qi], hreduce=mode, what=("six decades", mode, qi))
    assert idx.batched_filter_stats()["int8_queries"] == 600
    idx.close()


# ---- 5. the three reduce_add orders -----------------------------------------------------------------------------------------------

def test_f32_batched_equals_exact_equals_oracle_in_every_reduce_order(fa, oracle):
    dim, n = 256, 200_003
    rows, cent = corpus(dim, n)
    idx = fa.VectorIndex.from_slab_f32(rows)
    q = R.case_queries(dim, n, 255, 30, rows, cent)
    seen = []
    for mode in (0, 1, 2):
        idx.set_hreduce(mode)
        br, bs, bc, fb = idx.search_batched(q, 30)
        assert_same((br, bs, bc), exact_in_slices(idx, q, 30), ("hreduce", mode))
        assert fb <= 255 // 8 and "scan_wide_kernel" in main_pass_kernel(fa)
        for qi in (0, 1, 200, 254):
            assert_oracle(oracle, rows, q[qi], 30, br[qi], bs[qi], hreduce=mode, what=("hreduce", mode, qi))
        seen.append(bits(bs).copy())
    assert idx.batched_filter_stats()["int8_queries"] == 3 * 255
    assert not (np.array_equal(seen[0], seen[1]) and np.array_equal(seen[0], seen[2]))   # (the orders do differ somewhere)
    idx.close()


# ---- 6. pinned filters and gates --------------------------------------------------------------------------------------------------

def test_f32_pinned_filters_and_gates(fa, oracle):
    dim, n = 128, 33_001
    rows, cent = corpus(dim, n)
    q = R.case_queries(dim, n, 129, 10, rows, cent)
    idx = fa.VectorIndex.from_slab_f32(rows)
    want = exact_in_slices(idx, q, 10)
    br, bs, bc, fb = idx.search_batched(q, 10)
    assert_same((br, bs, bc), want, "automatic")
    assert idx.batched_filter_stats()["int8_queries"] == 129
    idx.set_batched_filter(1)       # "f16 filter" on an F32 index: no int8 filter, i.e. the exact f32 kernels
    br, bs, bc, fb = idx.search_batched(q, 10)
    assert_same((br, bs, bc), want, "pinned to f16")
    assert idx.batched_filter_stats()["int8_queries"] == 129 and fb == 129
    idx.set_batched_filter(2)
    br, bs, bc, fb = idx.search_batched(q[:3], 10)   # pinned to int8: even three queries
    assert_same((br, bs, bc), tuple(w[:3] for w in want), "pinned to int8")
    assert idx.batched_filter_stats()["int8_queries"] == 132
    want65 = exact_in_slices(idx, q, 65)
    br, bs, bc, fb = idx.search_batched(q, 65)       # k = 65: today's path
    assert_same((br, bs, bc), want65, "k = 65")
    assert idx.batched_filter_stats()["int8_queries"] == 132
    # the int8 two-pass stays F16-only: on an F32 index its batched form answers every query with the exact search, as the
    # reference falls back for quantization != F16 (search.rs:579-585) — no int8 filter copy involved, every query a fallback;
    # the F16-only ERROR is what a sharded handle's two-pass mode raises (test_f32_ride_alongs_on_an_fsvi_file)
    tr, ts, tc, tfb = idx.search_int8_two_pass_batched(q[:20], 10, 3)
    assert_same((tr, ts, tc), tuple(w[:20] for w in want), "int8 two-pass on F32")
    assert tfb == 20 and idx.batched_filter_stats()["int8_queries"] == 132
    idx.close()
    small = fa.VectorIndex.from_slab_f32(rows[:20_000])   # below the 32,768-row gate
    br, bs, bc, fb = small.search_batched(q, 10)
    assert_same((br, bs, bc), exact_in_slices(small, q, 10), "20,000 rows")
    assert small.batched_filter_stats()["int8_queries"] == 0
    assert_oracle(oracle, rows[:20_000], q[5], 10, br[5], bs[5], what="20,000 rows")
    small.close()


# ---- 7. the begin / end halves ----------------------------------------------------------------------------------------------------

def test_f32_two_tickets_in_flight_equal_the_blocking_call(fa):
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    dim, n = 256, 200_003
    rows, cent = corpus(dim, n)
    dev = torch.device("cuda", 0)
    slab = torch.from_numpy(rows).to(dev)
    idx = fa.VectorIndex.from_device_slab_f32(slab.data_ptr(), n, dim, keepalive=slab)
    be = GpuShardBackend(idx, dev, batched=True)
    qs = []
    for j, (nq, k) in enumerate(((255, 10), (640, 10), (129, 10))):
        q = R.case_queries(dim, n, nq, k, rows, cent)
        q[3] = 0.0                   # an uncertifiable query: answered by the exact f32 kernels in _end
        qs.append(torch.from_numpy(q).to(dev))
    want = [be.search_batched(q, 10) for q in qs]
    torch.cuda.synchronize()
    before = idx.batched_filter_stats()["int8_queries"]
    got, prev = [], None
    for q in qs:
        cur = be.scan_begin(q, 10, packed=False)     # two tickets in flight from the second begin on
        if prev is not None:
            assert be.scan_end(prev[1]) >= 1
            got.append(prev[0])
        prev = cur
    be.scan_end(prev[1])
    got.append(prev[0])
    torch.cuda.synchronize()
    assert idx.batched_filter_stats()["int8_queries"] - before == 255 + 640 + 129
    for j in range(len(qs)):
        for x, y in zip(got[j], want[j]):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), j
    # ... and the blocking call equals the exact kernels
    er, es, ec = exact_in_slices(idx, qs[0].cpu().numpy(), 10)
    assert np.array_equal(want[0][0].cpu().numpy().view(np.uint32), er) and np.array_equal(bits(want[0][1].cpu().numpy()), bits(es))
    idx.close()


# ---- 8. what rides along ----------------------------------------------------------------------------------------------------------

def test_f32_ride_alongs_on_an_fsvi_file(fa, oracle, tmp_path):
    import smooth_ref as SR
    rng = np.random.default_rng(808)
    n, dim, k = 100_003, 64, 10
    vec = R.unit_rows(rng, n, dim)
    ids = [f"doc-{i:06d}" for i in range(n)]
    path = str(tmp_path / "f32.fsvi")
    fa.write_fsvi(path, zip(ids, vec), "emb", "r1", quantization=0)
    g = fa.VectorIndex.open(path)
    raw = open(path, "rb").read()
    slab = np.frombuffer(raw[oracle.Fsvi(path).vectors_offset:], dtype="<f4").reshape(n, dim).copy()   # file order
    # (a) the k-NN graph self-join on a 2,048-source slice: 16 sampled sources against the oracle with the self rule
    m = 10
    first = 50_000
    krows, ksims = g.build_knn_graph(m, first_row=first, n_rows=2048, want_sims=True)
    assert g.batched_filter_stats()["int8_queries"] >= 2048, "the self-join did not ride the int8-filtered matrix path"
    for s in rng.choice(2048, 16, replace=False):
        orow, osc = oracle.search_top_k_f32(slab, slab[first + s], m + 1)
        kept = SR.knn_from_topk([int(x) for x in orow], int(first + s), m)
        score_of = {int(r): sc for r, sc in zip(orow, osc)}
        assert [int(x) for x in krows[s]] == list(kept), s
        assert np.array_equal(bits(ksims[s]), bits([score_of[r] for r in kept])), s
    # (b) the sharded handle on one device: batched search == the unsharded index
    q = (slab[rng.integers(0, n, 32)] + (0.3 * rng.standard_normal((32, dim))).astype(F32)).astype(F32)
    many = np.tile(q, (5, 1))[:150]
    sh = fa.NativeShardedIndex.open(path, [0, 0, 0])
    sr, ss, sc_ = sh.search_batch(many, k, batched=True)[:3]
    ur, us, uc, _ = g.search_batched(many, k)
    assert np.array_equal(sr, ur) and np.array_equal(bits(ss), bits(us)) and np.array_equal(sc_, uc)
    from frankensearch_amd.errors import SearchError as FsgpuError
    with pytest.raises(FsgpuError, match="F16"):          # the two-pass searches still refuse F32 with the F16-only error
        sh.search(many[:20], k, fa.NativeShardedIndex.INT8_TWO_PASS, candidate_multiplier=3)
    sr2, ss2, sc2 = sh.search_batch(many, k, batched=True)[:3]   # ... and the handle goes on answering
    assert np.array_equal(sr2, ur) and np.array_equal(bits(ss2), bits(us)) and np.array_equal(sc2, uc)
    sh.close()
    # (c) search_hits_batched with 40 tombstones and 25 WAL entries == the per-query search_hits
    dead = [ids_i for ids_i in (g.doc_id_at(int(r)) for r in rng.choice(n, 40, replace=False))]
    for d in dead:
        assert g.soft_delete(d)
    g.append_batch([(f"wal-{j:02d}", (q[j] * F32(1.0 + 0.01 * j)).tolist()) for j in range(25)])
    assert g.wal_record_count() == 25
    before = g.batched_filter_stats()["int8_queries"]
    batch = g.search_hits_batched(q, k)
    assert g.batched_filter_stats()["int8_queries"] - before == 32
    for qi in range(32):
        lone = g.search_top_k(q[qi], k)
        assert [(h.index, h.doc_id) for h in batch[qi]] == [(h.index, h.doc_id) for h in lone], qi
        assert np.array_equal(bits([h.score for h in batch[qi]]), bits([h.score for h in lone])), qi
    assert any(h.doc_id.startswith("wal-") for h in batch[0])
    g.close()


# ---- 9. repeatability --------------------------------------------------------------------------------------------------------------

def test_f32_the_same_batch_fifty_times_gives_identical_bits(fa):
    dim, n = 256, 262_163
    rows, cent = corpus(dim, n)
    idx = fa.VectorIndex.from_slab_f32(rows)
    q = R.case_queries(dim, n, 1030, 10, rows, cent)
    first = idx.search_batched(q, 10)
    for rep in range(49):
        again = idx.search_batched(q, 10)
        assert np.array_equal(again[0], first[0]) and np.array_equal(bits(again[1]), bits(first[1])) and np.array_equal(again[2], first[2]), rep
    assert idx.batched_filter_stats()["int8_queries"] == 50 * 1030
    idx.close()

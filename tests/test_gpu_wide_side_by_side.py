"""The two layouts of the register-resident-query main pass (mfma_wide.hip; vector_index_batched.cpp: batched_main).

A main-pass launch that carries G query groups runs them SIDE BY SIDE — G x (grid / G) blocks, all resident, walker w of every
group on the same row tiles at the same time, so the slab leaves HBM once per launch — where it used to run them one after the
other on the whole grid (FSGPU_WIDE_LAYOUT=sequential keeps that layout; it is also what one group, a grid the groups do not
divide, or a slab of a few tiles per walker get).  The layout moves blocks, lists and the order rows are visited in; it must not
move an answer.  For 512 / 768 / 1,000 / 1,024 / 2,048 queries at 256 and 384 dimensions, on a slab whose tile count is ragged
against the walker count, with a tombstone bitmap + an allow bitmap + a non-zero row base, and for the int8 two-pass:
rows, f32 score bits and counts of the batched search equal the exact kernels', and equal the sequential layout's — computed by
a child process of this file under FSGPU_WIDE_LAYOUT=sequential (the switch is read once per process).
"""
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = 10
# 70,001 rows: 547 tiles of 128 rows (1,094 of 64) over 128 walkers — 4.27 (8.5) rounds, first and last ragged; above the
# 4 x 128 x walkers rows a launch needs to run side by side on a 256-CU part
N_PLAIN = 70_001
N_MASKED = 90_007
ROW_BASE = 3_000_000
QUERY_COUNTS = (512, 768, 1000, 1024, 2048)
DIMS = (256, 384)
TWO_PASS_SAMPLE = (0, 1, 255, 256, 511, 512, 777, 1023)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def corpus(seed, n, dim):
    """Clustered unit-ish rows (many rows within reach of a query's k-th best: the lists fill) and queries near rows."""
    rng = np.random.default_rng(seed)
    cent = rng.standard_normal((64, dim)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    rows = cent[rng.integers(0, 64, n)] + (0.7 / np.sqrt(dim)) * rng.standard_normal((n, dim)).astype(np.float32)
    slab = rows.astype(np.float16)
    nq = max(QUERY_COUNTS)
    q = rows[rng.integers(0, n, nq)] + (0.5 / np.sqrt(dim)) * rng.standard_normal((nq, dim)).astype(np.float32)
    return slab, q.astype(np.float32), rng


def masks(rng, n):
    live = rng.random(n) >= 0.07       # 7 % tombstones
    allow = rng.random(n) < 0.6
    return live, allow


def batched_answers(fa, dim):
    """Every batched search of this file for one dimension: {name: (rows, scores, counts, fallbacks)}."""
    out = {}
    slab, q, _ = corpus(100 + dim, N_PLAIN, dim)
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16))
    for nq in QUERY_COUNTS:
        out[f"plain_{nq}"] = idx.search_batched(q[:nq], K)
    out["two_pass"] = idx.search_int8_two_pass_batched(q[:1024], K, 3)
    idx.close()
    slab, q, rng = corpus(200 + dim, N_MASKED, dim)
    live, allow = masks(rng, N_MASKED)
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16), live=live, row_base=ROW_BASE)
    out["masked_1024"] = idx.search_batched(q[:1024], K, allow=allow)
    idx.close()
    return out


def _child(path):
    assert os.environ.get("FSGPU_WIDE_LAYOUT") == "sequential"
    sys.path.insert(0, ROOT)
    import frankensearch_amd as fa

    arrays = {}
    for dim in DIMS:
        for name, (rows, scores, counts, fb) in batched_answers(fa, dim).items():
            arrays[f"{dim}_{name}_rows"] = rows
            arrays[f"{dim}_{name}_scores"] = bits(scores)
            arrays[f"{dim}_{name}_counts"] = counts
            arrays[f"{dim}_{name}_fallbacks"] = np.array([fb], np.uint32)
    np.savez(path, **arrays)


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    assert fa_mod._lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    assert "FSGPU_WIDE_LAYOUT" not in os.environ, "this process must run the default layout"
    return fa_mod


@pytest.fixture(scope="module")
def sequential(fa, tmp_path_factory):
    """The same searches under the sequential layout, from a fresh process."""
    path = str(tmp_path_factory.mktemp("wide_layout") / "sequential.npz")
    env = dict(os.environ, FSGPU_WIDE_LAYOUT="sequential")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return np.load(path)


@pytest.fixture(scope="module", params=DIMS)
def side(request, fa):
    dim = request.param
    return dim, batched_answers(fa, dim)


def same_as_sequential(sequential, dim, name, got):
    rows, scores, counts, fb = got
    print(f"dim {dim} {name}: fallbacks side by side {fb}, sequential {int(sequential[f'{dim}_{name}_fallbacks'][0])}")
    assert np.array_equal(counts, sequential[f"{dim}_{name}_counts"]), (dim, name)
    assert np.array_equal(rows, sequential[f"{dim}_{name}_rows"]), (dim, name)
    assert np.array_equal(bits(scores), sequential[f"{dim}_{name}_scores"]), (dim, name)


@pytest.mark.parametrize("nq", QUERY_COUNTS)
def test_plain_batches_equal_the_exact_kernels_and_the_sequential_layout(fa, side, sequential, nq):
    dim, answers = side
    slab, q, _ = corpus(100 + dim, N_PLAIN, dim)
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16))
    er, es, ec = idx.search_batch(q[:nq], K, exact=True)
    idx.close()
    rows, scores, counts, _ = answers[f"plain_{nq}"]
    assert np.all(ec == K)
    assert np.array_equal(counts, ec)
    assert np.array_equal(rows, er)
    assert np.array_equal(bits(scores), bits(es))
    same_as_sequential(sequential, dim, f"plain_{nq}", answers[f"plain_{nq}"])


def test_tombstones_allow_bitmap_and_row_base(fa, side, sequential):
    dim, answers = side
    slab, q, rng = corpus(200 + dim, N_MASKED, dim)
    live, allow = masks(rng, N_MASKED)
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16), live=live, row_base=ROW_BASE)
    er, es, ec = idx.search_batch(q[:1024], K, allow=allow, exact=True)
    idx.close()
    rows, scores, counts, _ = answers["masked_1024"]
    assert np.all(ec == K)
    local = er.astype(np.int64) - ROW_BASE   # the hits are global rows of live, allowed local rows
    assert local.min() >= 0 and local.max() < N_MASKED and np.all(live[local]) and np.all(allow[local])
    assert np.array_equal(counts, ec)
    assert np.array_equal(rows, er)
    assert np.array_equal(bits(scores), bits(es))
    same_as_sequential(sequential, dim, "masked_1024", answers["masked_1024"])


def test_int8_two_pass_equals_the_per_query_search_and_the_sequential_layout(fa, side, sequential):
    dim, answers = side
    slab, q, _ = corpus(100 + dim, N_PLAIN, dim)
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16))
    rows, scores, counts, _ = answers["two_pass"]
    for qi in TWO_PASS_SAMPLE:
        hits = idx.search_top_k_int8_two_pass(q[qi], K, 3)
        assert int(counts[qi]) == len(hits) == K
        assert [h.index for h in hits] == rows[qi].tolist(), qi
        assert np.array_equal(bits(np.array([h.score for h in hits], np.float32)), bits(scores[qi])), qi
    idx.close()
    same_as_sequential(sequential, dim, "two_pass", answers["two_pass"])


if __name__ == "__main__":
    _child(sys.argv[1])

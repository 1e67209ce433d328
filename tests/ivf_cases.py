"""Fixtures of the IVF index's tests, shared by the GPU tests (test_gpu_ivf.py) and the checks that need no GPU
(test_ivf_contract.py).  numpy and tests/ivf_ref.py only; the library and the oracle come in as arguments.  Each fixture aims at
one rule of the contract (include/fsgpu.h, "IVF index") and test_ivf_contract.py shows that it does reach it."""
import numpy as np

import ivf_ref as R

F32 = np.float32

# ---- the caps, from kernels.hpp's constants -------------------------------------------------------------------------------------
GATHER_MAX_K, GATHER_TILE_ROWS, GATHER_LDS_BUDGET, WAVES_PER_BLOCK = 256, 64, 160 * 1024, 4
MAX_LISTS, MAX_PROBE, MAX_ITERS, MERGE_MAX_ENTRIES = 65536, 256, 64, 16384


def gather_row_pitch(dim):
    return (dim * 2 + 255 - 64) // 256 * 256 + 64


def gather_lds_bytes(dim, kcap):
    """filter_gather_lds_bytes (filter_gather_kernels.hip): the tile, a query and a candidate buffer per wave, the tile's row ids."""
    return GATHER_TILE_ROWS * gather_row_pitch(dim) + WAVES_PER_BLOCK * dim * 4 + WAVES_PER_BLOCK * 2 * kcap * 8 + GATHER_TILE_ROWS * 4


def gather_supported(dim, k):
    return dim >= 8 and dim % 8 == 0 and 1 <= k <= GATHER_MAX_K and gather_lds_bytes(dim, 64 if k <= 64 else 256) <= GATHER_LDS_BUDGET


def call_ok(dim, nlist, k, nprobe):
    return gather_supported(dim, k) and 1 <= nprobe <= min(nlist, MAX_PROBE) and nprobe * k <= MERGE_MAX_ENTRIES


# ---- corpora ----------------------------------------------------------------------------------------------------------------------

def f16(rows_f32):
    return np.ascontiguousarray(rows_f32, dtype=F32).astype(np.float16).view(np.uint16)


def normal_rows(seed, n, dim):
    return f16(np.random.default_rng(seed).standard_normal((n, dim)))


def one_in_seven_dead(n):
    live = np.ones(n, dtype=bool)
    live[3::7] = False
    return live


def duplicate_corpus(dim=16):
    """64 distinct unit rows, each 50 times in a run; nlist 128 with the strided init takes rows 25 c, i.e. distinct row c // 2: centroids
    2 j and 2 j + 1 are equal, every row ties between them, the lower id takes it; the higher list is empty in the first iteration
    and keeps its bits through it."""
    distinct = np.random.default_rng(7).standard_normal((64, dim)).astype(F32)
    distinct /= np.linalg.norm(distinct, axis=1, keepdims=True)   # unit rows: a row's best centroid is its own
    return f16(np.repeat(distinct, 50, axis=0)), 128


def underfill_corpus(dim=16, n=400):
    """Rows 0 .. n - 4 lie around +e0, the last three rows around +e1; the caller's two centroids are e0 and e1.  The query e1 probes
    list 1 alone: 3 rows at k = 10.  Deleting those three rows after the build leaves the probed list wholly dead."""
    rng = np.random.default_rng(11)
    rows = 0.05 * rng.standard_normal((n, dim)).astype(F32)
    rows[:n - 3, 0] += 1.0
    rows[n - 3:, 1] += 1.0
    init = np.zeros((2, dim), dtype=F32)
    init[0, 0] = init[1, 1] = 1.0
    query = np.zeros(dim, dtype=F32)
    query[1] = 1.0
    return f16(rows), init, query, np.arange(n - 3, n)


def nonfinite_corpus(dim=16, n=600):
    """Random rows; rows 5 and 17 hold a NaN (every score NaN: list 0, whose mean is then not finite), row 40 a +inf, row 41 a -inf
    (their lists' sums are infinite).  nlist 8 with the strided init takes rows 0, 75, 150, ...: all finite."""
    rows = np.random.default_rng(13).standard_normal((n, dim)).astype(F32)
    rows[5, 2] = np.nan
    rows[17, 9] = np.nan
    rows[40, 3] = np.inf
    rows[41, 5] = -np.inf
    return f16(rows), 8


def cancelling_corpus(dim=8, big=20000, tiny=10000):
    """One list whose f64 sums depend on the ORDER of the additions: `big` rows of values in [30,000, 65,504] (their sum passes
    2^30, where an f64 has 2^-22 to spare), `tiny` rows of f16 subnormals (multiples of 2^-24), then the big rows negated, which
    cancel exactly.  What is left is the tiny rows' sum as the big partial sum rounded it: nlist 1, iters 1."""
    rng = np.random.default_rng(17)
    large = rng.uniform(30000.0, 65504.0, size=(big, dim)).astype(np.float16)
    small = (rng.integers(1, 1024, size=(tiny, dim)).astype(np.uint16)).view(np.float16)   # subnormals, as bit patterns
    return np.ascontiguousarray(np.concatenate([large, small, -large])).view(np.uint16), 1


def clustered(oracle, n=16384, dim=64, nq=200):
    slab = oracle.clustered_corpus_f16(0, n, dim)
    queries = np.stack([oracle.clustered_query(q, dim) for q in range(nq)])
    return slab, queries


CERT = dict(nlist=64, iters=4, candidates=(1, 2, 4, 8, 16, 32), k=10, target=0.95, alpha=0.1)


def exact_rows(oracle, slab, queries, k, live=None, hreduce=0):
    return [oracle.search_top_k(slab, q, k, live=live, hreduce=hreduce)[0] for q in queries]


def score_table(oracle, slab, queries, hreduce=0):
    """[nq, N] exact scores of every row."""
    every = np.arange(slab.shape[0], dtype=np.uint32)
    return np.stack([oracle.gather_dot(slab, q, every, hreduce) for q in queries])


def exact_from_scores(row_scores):
    """An exact search over a precomputed score row, in the reference's order."""
    def exact(query, k, live):
        cand = np.nonzero(live)[0].astype(np.uint32)
        order = np.argsort(R.order_keys(row_scores[cand], cand), kind="stable")[::-1][:k]
        return cand[order], row_scores[cand][order]
    return exact

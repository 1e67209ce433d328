"""Fixtures of the IVF index's tests, shared by the GPU tests (test_gpu_ivf.py, test_gpu_ivf_shapes.py) and the checks that need no GPU
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


# ---- the assignment's tile, from kernels.hpp's and join_tile.hpp's constants -------------------------------------------------------
JOIN_ROWS_PER_WAVE, JOIN_CHUNK, IVF_LDS_BUDGET, IVF_LAUNCH_ROWS = 16, 16, 159 * 1024, 1 << 20
ASSIGN_FIXED_DIMS = (384, 256, 128, 64)
KNN_MAX_M, KNN_UPD_MAX_DIM = 63, 1024   # the coarse step is the transposed join from 16 queries on, up to these


def join_tile_plan(dim, budget=IVF_LDS_BUDGET, fixed_dims=ASSIGN_FIXED_DIMS, extra_per_wave=0):
    """plan_join_tile (join_tile.hpp) -> (waves, xstride, qstride, lds bytes, fixed): four waves of 16 rows, halved until the rows
    and a chunk of 16 streamed vectors fit the budget; lds 0: even one wave does not fit; fixed: the compile-time dimension applies."""
    xstride, qstride = ((dim + 15) & ~15) + 8, (dim + 1) & ~1
    fixed = dim in fixed_dims
    if fixed:
        qstride = dim

    def lds_of(waves):
        return (waves * JOIN_ROWS_PER_WAVE * xstride + JOIN_CHUNK * qstride) * 4 + waves * extra_per_wave
    waves = 4
    while waves > 1 and lds_of(waves) > budget:
        waves >>= 1
    lds = 0 if lds_of(waves) > budget else lds_of(waves)
    return waves, xstride, qstride, lds, fixed and waves == 4


def assign_supported(dim):
    """ivf_assign_supported (ivf_kernels.hip)."""
    return dim >= 8 and dim % 8 == 0 and join_tile_plan(dim)[3] != 0


def build_supported(dim):
    """IvfIndex::init's gate on the dimension: the assignment's tile AND the gather scan's (k = 1) fit their LDS."""
    return assign_supported(dim) and gather_supported(dim, 1)


def wave_ladder():
    """The dimensions at which the assignment changes its form -> {name: dim}: the last with four waves, the first with two, the
    first with one, the largest a build accepts and the first it refuses.  The gather scan's tile gives out before the
    assignment's (test_ivf_contract.py shows it), so the last two are build_supported's, not assign_supported's."""
    dims = range(8, 4096, 8)
    waves = {d: join_tile_plan(d)[0] for d in dims if assign_supported(d)}
    return dict(last4=max(d for d, w in waves.items() if w == 4), first2=min(d for d, w in waves.items() if w == 2),
                first1=min(d for d, w in waves.items() if w == 1), largest=max(d for d in dims if build_supported(d)),
                refused=min(d for d in dims if not build_supported(d)))


def coarse_is_join(nq, nprobe, dim):
    """IvfIndex::search: the transposed join answers the coarse step, else the F32 index over the centroids."""
    return nq >= 16 and nprobe <= KNN_MAX_M and dim <= KNN_UPD_MAX_DIM


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


def hashmix(oracle, n=4099, dim=64):
    return f16(oracle.fixture_hashmix(n, dim))


def noisy_queries(slab, nq, seed, noise=0.1):
    """nq distinct rows of the slab, widened, plus noise."""
    rng = np.random.default_rng(seed)
    pick = rng.choice(slab.shape[0], nq, replace=False)
    return (R.widen(slab[pick]) + noise * rng.standard_normal((nq, slab.shape[1]))).astype(F32)


def two_launch_corpus(dim=8, extra=300):
    """The assignment runs in launches of IVF_LAUNCH_ROWS rows: 2^20 + 300 rows make a second launch with row0 = 2^20, whose 300 rows
    are four whole 64-row tiles and one of 44.  One row in seven is dead, and so is a run of 200 rows across row 2^20: the last
    two tiles of the first launch hold no gated row, and the first tile of the second launch only its last 14 rows.  (The dead rows are 5 mod 7: a sample of 5,000
    training rows steps by 209.8 rows, close to 30 x 7, and its last rows, the only ones past 2^20, are all 3 mod 7.)
    -> (slab, live, nlist 3)"""
    n = IVF_LAUNCH_ROWS + extra
    live = np.ones(n, dtype=bool)
    live[5::7] = False
    live[IVF_LAUNCH_ROWS - 150:IVF_LAUNCH_ROWS + 50] = False
    return normal_rows(19, n, dim), live, 3


def dead_tiles_live(n=4099):
    """Rows 256 .. 767 dead: eight whole 64-row workgroups of the assignment (which has 64 rows per workgroup at dim 64) without
    a gated row, whose rows keep the 0xff prefill of the assignment and must stay out of every list."""
    live = np.ones(n, dtype=bool)
    live[256:768] = False
    return live


DEAD_TILES = dict(nlist=7, iters=2, n_train=40)   # n_train 40 over 4,099 rows: a training row per ~102 rows, most tiles ungated


def empty_ends_init(slab, nlist=5):
    """A caller's centroids whose FIRST and LAST list take no row: centroids 1 and 2 are v and -v (one of the two scores is > 0
    unless both are 0), centroid 3 is another row, and centroids 0 and nlist - 1 are v / 1024, whose score is the 1024th of v's in
    size: below the better of v and -v."""
    wide = R.widen(slab)
    init = np.zeros((nlist, slab.shape[1]), dtype=F32)
    init[1], init[2] = wide[0], -wide[0]
    for c in range(3, nlist - 1):
        init[c] = wide[c * 100]
    init[0] = init[nlist - 1] = wide[0] / F32(1024.0)
    return init


ONE_TILE = dict(nlist=300, iters=0, nq=33, ks=(1, 10, 64, 65, 256), nprobes=(1, 5, 63, 64, 256))


def one_tile_corpus(oracle, which):
    """4,099 rows x 64, one in seven dead, for nlist 300 with the strided init.  "normal": random rows, every list has 1 .. 64 rows —
    one 64-row tile, so every probed list has one scan block and the per-query merge reads the scan's own table — and many are
    shorter than 10.  "hashmix": the hashmix rows lie in a few dozen bundles; 255 of the 300 lists are empty and the others have up
    to 119 rows: probed empty lists by the hundred beside lists of two tiles.  -> (slab, live)"""
    slab = hashmix(oracle) if which == "hashmix" else normal_rows(64, 4099, 64)
    return slab, one_in_seven_dead(4099)


def duplicate_queries(noise=0.01):
    """The 64 distinct rows of duplicate_corpus() plus a little noise: query c's two best centroids are the twins 2 c and 2 c + 1,
    and the higher twin's list is empty."""
    slab, _ = duplicate_corpus()
    rng = np.random.default_rng(29)
    return (R.widen(slab[::50]) + noise * rng.standard_normal((64, slab.shape[1]))).astype(F32)


def ragged_cases():
    """nlist 17, 19 and 100 are no multiples of the join's chunk of 16 centroids: the last chunk is ragged in the transposed join
    (16 queries and more, nprobe <= 63) and the centroid index's last tile in the other form.  -> [(dim, nlist, hreduce)], the
    hreduce order rotated over the cases."""
    return [(dim, nlist, (i + j) % 3) for i, dim in enumerate((64, 128, 256, 72)) for j, nlist in enumerate((17, 19, 100))]


RAGGED = dict(n=3000, iters=1, nqs=(15, 16, 257), nprobes=(1, 17, 63, 64), k=10)


def nonfinite_queries(slab, nq, at):
    """Noisy queries with three replaced at positions `at`: one with a NaN (every score NaN), one with a +inf (scores +inf, -inf
    or NaN), the all-zero query (every score a zero: the lower id first)."""
    q = noisy_queries(slab, nq, 31)
    q[at[0], 3] = np.nan
    q[at[1], 7] = np.inf
    q[at[2]] = 0.0
    return q


NONFINITE_Q = dict(nlist=16, iters=2, nq=19, at=(2, 9, 17), k=10, nprobe=5)   # over the 4,099 hashmix rows, one in seven dead


# ---- the coarse step over many centroids ------------------------------------------------------------------------------------------
MFMA_DIMS, I8F_MIN_ROWS, I8F_MAX_K, I8F_BUILD_MIN_QUERIES = (64, 128, 256, 384), 4 * 8192, 64, 16


def coarse_by_int8_filter(nlist, dim, nq, nprobe, filter_ready):
    """VectorIndex::batched_exact's gate for the centroid index (an F32 slab, k = nprobe) when the join does not take the call:
    the int8 matrix-core filter answers at a dimension the matrix-core scan serves, from 32,768 rows, up to k = 64 — and below 16
    queries only once an earlier call has built the int8 copy.  Everything else is the exact F32 kernels."""
    return (not coarse_is_join(nq, nprobe, dim) and dim in MFMA_DIMS and nlist >= I8F_MIN_ROWS and 1 <= nprobe <= I8F_MAX_K
            and (nq >= I8F_BUILD_MIN_QUERIES or filter_ready))


# 50,000 rows, every list a row or two; the calls IN THIS ORDER: (nq, nprobe).  At dim 64 the first builds and uses the int8 copy, the
# next two find it ready, the last is the join; at dim 16, which the matrix-core scan does not serve, the first three are the exact
# F32 kernels over 40,000 centroids
MANY_LISTS = dict(n=50000, nlist=40000, iters=0, k=10, calls=((40, 64), (8, 64), (8, 5), (40, 5)), dims=(64, 16))


def many_lists_corpus(dim):
    return normal_rows(41 + dim, MANY_LISTS["n"], dim)


WIDE = dict(n=1500, nlist=12, iters=1, nq=20, dims=(520, 1000), ks=(10, 64), nprobes=(1, 5, 12))


def wide_corpus(dim):
    """Rows wider than the join's fixed dimensions: 520 (two waves in the assignment, served by the gather scan up to k = 256) and
    1000 (one wave; the scan's 256-entry buffers do not fit: k <= 64 only).  -> (slab, hreduce)"""
    return normal_rows(dim, WIDE["n"], dim), 1 if dim == 520 else 2


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

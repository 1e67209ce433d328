"""Helpers and hand-made cases of the graph ANN search's tests, shared by the GPU tests (test_gpu_ann.py, test_gpu_ann_shapes.py) and
the checks that need no GPU (test_ann_contract.py).  numpy and tests/ann_ref.py only; the library and the oracle come in as arguments.

The search is defined for ANY [n, width] table, so the cases below make their tables by hand — no k-NN build, every dimension the
index accepts is reachable — and each one aims at code that random rows over a built table never run (ann_kernels.hip)."""
import numpy as np

import ann_ref as R

F32 = np.float32
PAD = R.PAD

# the default hand-made case: a seeded random table, 64 entry rows so that the steps really walk
N, WIDTH, NQ, N_ENTRY = 2048, 16, 9, 64
K_EF = ((10, 64), (16, 16))

# quad_dot_f16<12> (ann_kernels.hip): `vec` needs dim % 8 == 0 (whole 16-byte chunks, 16-byte rows); groups = dim // 32, leftover
# chunks = dim // 8 % 4, tail = dim % 8.   dim: (groups, leftover chunks, tail)
F16_VECTOR_DIMS = {8: (0, 1, 0), 24: (0, 3, 0), 40: (1, 1, 0), 72: (2, 1, 0), 416: (13, 0, 0), 792: (24, 3, 0)}   # 13, 24 > BATCH 12
F16_ELEMENT_DIMS = {4: (0, 0, 4), 7: (0, 0, 7), 43: (1, 1, 3), 397: (12, 1, 5)}
# quad_dot_f32<6> (scan_common.hpp): `vec` needs a row stride of whole 16 bytes, dim % 4 == 0
F32_VECTOR_DIMS = {8: (0, 1, 0), 24: (0, 3, 0), 40: (1, 1, 0), 200: (6, 1, 0), 232: (7, 1, 0)}                     # 7 > BATCH 6
F32_ELEMENT_DIMS = {7: (0, 0, 7), 43: (1, 1, 3), 99: (3, 0, 3)}
ALL_HREDUCE_DIMS = (40, 43, 416)

# LDS of ann_search_kernel = the query as f32, rounded up to 16 bytes, + the state behind it.  The state, from the kOff* constants of
# ann_kernels.hip (kAnnMaxEf 256, kAnnMaxStepRows 512, kAnnTableSlots 8192):
#   beam 2 x 256 x 8 = 4,096 | cand 512 x 8 = 4,096 | table 8,192 x 4 = 32,768 | walk 512 x 4 = 2,048 | admit 512 x 4 = 2,048 |
#   flags 2 x 256 = 512 | small 24 x 4 = 96                                                             -> 45,664 bytes
# 65,536 - 45,664 = 19,872 = 4 x 4,968: dimension 4,968 is exactly 64 KB (hipFuncSetAttribute NOT called: `lds > 64 KB` is false),
# 4,969 .. 4,972 round to 19,888 and are the first above it; 4,976 is the first multiple of 8 above it.  kAnnMaxDim = 16,384 needs
# 65,536 + 45,664 = 111,200 bytes of the 160 KB.
ANN_STATE_BYTES = 2 * 256 * 8 + 512 * 8 + 8192 * 4 + 512 * 4 + 512 * 4 + 2 * 256 + 24 * 4
ANN_MAX_DIM = 16384


def ann_lds_bytes(dim):
    return ((dim * 4 + 15) & ~15) + ANN_STATE_BYTES


LDS_DIMS = (4968, 4976, ANN_MAX_DIM)   # F16; one F32 case at 4,976
LDS_N, LDS_NQ = 512, 5


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def tombstones(rng, n, n_entry=256):
    """10 % of the rows, some of them entry rows of the strided entry set."""
    live = np.ones(n, dtype=bool)
    live[rng.choice(n, size=n // 10, replace=False)] = False
    live[np.asarray(R.entry_rows(n, n_entry))[[3, 5, 100]]] = False
    live[0] = True   # (the one entry row of n_entry = 1)
    return live


def score_table(oracle, slab, queries, f32, hreduce):
    """[nq, N] exact scores of every row, by the CPU oracle."""
    n = slab.shape[0]
    out = np.empty((len(queries), n), dtype=F32)
    every = np.arange(n, dtype=np.uint32)
    for i, q in enumerate(queries):
        if f32:
            rows, scores = oracle.search_top_k_f32(slab, q, n, hreduce=hreduce)   # k = N: every row with its score
            assert rows.size == n
            out[i, rows] = scores
        else:
            out[i] = oracle.gather_dot(slab, q, every, hreduce)
    return out


def assert_device_is_reference(ann, table, scores, live, queries, k, ef, cfg, row_base, what):
    rows, sc, counts, flags = ann.search_batched(queries, k, ef)
    st = ann.stats
    live_rows = int(live.sum()) if live is not None else scores.shape[1]
    bad, want_scored, want_steps = [], 0, 0
    for i in range(len(queries)):
        wr, ws, wc, scored, steps = R.search(scores[i], live, table, k, ef, row_base=row_base, **cfg)
        want_scored += scored
        want_steps += steps
        assert R.flag_of(wc, k, live_rows) == R.APPROXIMATE, "the case was meant to stay on the approximate path"
        if counts[i] != wc or flags[i] != 0 or (rows[i, :wc] != wr).any() or (bits(sc[i, :wc]) != bits(ws)).any():
            bad.append(i)
    print(f"{what}: k {k} ef {ef} {cfg}: {len(queries)} queries, differing {len(bad)}, rows scored {st.rows_scored}, steps {st.steps}")
    assert not bad, (what, bad[:5], rows[bad[0]], counts[bad[0]])
    assert (st.rows_scored, st.steps) == (want_scored, want_steps)
    assert (st.queries, st.approximate, st.underfilled, st.empty_despite_indexed_points) == (len(queries), len(queries), 0, 0)
    assert (st.index_size, st.ef_search, st.k_requested, st.launches) == (scores.shape[1], ef, k, 1)


# ---- slabs and tables -----------------------------------------------------------------------------------------------------------------

def off_f16_grid(rng, half):
    """An F32 slab near the f16 rows whose values are not f16 values (the F32 slab of test_gpu_ann.make_case)."""
    return (half.astype(F32) * F32(1.0009765625) + rng.standard_normal(half.shape).astype(F32) * F32(1e-4)).astype(F32)


def hand_table(rng, n, width, live, row_base=0, without=()):
    """[n, width] global ids: every list `width` distinct random live rows, none of `without`."""
    ok = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool).copy()
    ok[list(without)] = False
    pool = np.flatnonzero(ok)
    assert pool.size >= width
    pick = np.argpartition(rng.random((n, pool.size)), width - 1, axis=1)[:, :width]
    return (pool[pick] + row_base).astype(np.uint32)


def dot_case(dim, f32, n=N, nq=NQ):
    """Seeded unit rows and queries, tombstones and a random table: the case of the dot-form and LDS tests."""
    rng = np.random.default_rng(1000 * dim + (7 if f32 else 0))
    half = R.unit_rows(rng, n, dim).astype(np.float16)
    queries = R.unit_rows(rng, nq, dim)
    live = tombstones(rng, n)
    slab = off_f16_grid(rng, half) if f32 else half.view(np.uint16)
    return dict(slab=slab, queries=queries, live=live, table=hand_table(rng, n, WIDTH, live), f32=f32, row_base=0)


def plain_dot(slab, queries, f32):
    """[nq, n] f32 dots accumulated left to right with a separate multiply and add — the order a kernel would have if it ignored
    the reference's eight accumulators, quad combine and horizontal add."""
    x = np.ascontiguousarray(slab).view(np.float16).astype(F32) if not f32 else np.ascontiguousarray(slab, dtype=F32)
    out = np.zeros((len(queries), x.shape[0]), dtype=F32)
    for j in range(x.shape[1]):
        out = (out + (x[None, :, j] * queries[:, j, None]).astype(F32)).astype(F32)
    return out


# ---- the hostile table (ann_kernels.hip: "every table, list and row index is checked against nrows before it is used") --------------

HOSTILE_CFGS = (dict(n_entry=N_ENTRY), dict(n_entry=N_ENTRY, expand=8, max_iters=32), dict(n_entry=N_ENTRY, degree=8))


def hostile_case(row_base):
    """A random table doctored row by row (a seeded pattern 0 .. 15 per row; 9 .. 15 stay random):
      every row   column 1 names X0 — the same id in every list a step expands (the `old == row` exit of the compare-and-swap loop);
                  X0's vector is query 0, so it leads query 0's answer and a walk that admitted it twice would show it twice;
                  column 8 names one of four shared rows
      0           a pad at column 0, Y0 behind it at column 2     Y0's vector is query 1 and no list names Y0 before a pad: a walk
      1           a pad at column 3, Y0 behind it at column 5     that read past a pad would put Y0 on top of query 1's answer
      2           a pad at the last column
      3           ids row_base + n, row_base + n + 5 and 0xFFFFFFFE
      4           ids 0 and 999 (below a row_base of 1,000: the subtraction wraps; plain rows at row_base 0)
      5           the row itself
      6           column 0's id again at columns 6 and 9
      7           a live entry row and a dead entry row
      8           two dead rows that are no entry rows"""
    rng = np.random.default_rng(77)
    n, dim = N, 64
    half = R.unit_rows(rng, n, dim).astype(np.float16)
    queries = R.unit_rows(rng, NQ, dim)
    live = tombstones(rng, n)
    entry = np.asarray(R.entry_rows(n, N_ENTRY))
    is_entry = np.zeros(n, dtype=bool)
    is_entry[entry] = True
    plain = np.flatnonzero(live & ~is_entry)
    x0, y0, *shared = (int(r) for r in rng.choice(plain, 6, replace=False))
    half[x0] = queries[0].astype(np.float16)
    half[y0] = queries[1].astype(np.float16)
    t = hand_table(rng, n, WIDTH, live, row_base, without=[x0, y0] + shared)
    g = lambda r: np.uint32(int(r) + row_base)
    live_entry, dead_entry = entry[live[entry]], entry[~live[entry]]
    dead_plain = np.flatnonzero(~live & ~is_entry)
    assert dead_entry.size >= 2 and dead_plain.size >= 2
    pattern = rng.integers(0, 16, n)
    pattern[[x0, y0]] = 15
    assert y0 not in (0, 999)
    t[:, 1] = g(x0)
    t[:, 8] = np.asarray(shared, dtype=np.uint32)[np.arange(n) % 4] + np.uint32(row_base)
    for r in range(n):
        p = pattern[r]
        if p == 0:
            t[r, 0], t[r, 2] = PAD, g(y0)
        elif p == 1:
            t[r, 3], t[r, 5] = PAD, g(y0)
        elif p == 2:
            t[r, WIDTH - 1] = PAD
        elif p == 3:
            t[r, 2], t[r, 7], t[r, 11] = row_base + n, row_base + n + 5, 0xFFFFFFFE
        elif p == 4:
            t[r, 4], t[r, 5] = 0, 999
        elif p == 5:
            t[r, 4] = g(r)
        elif p == 6:
            t[r, 6] = t[r, 9] = t[r, 0]
        elif p == 7:
            t[r, 3], t[r, 6] = g(rng.choice(live_entry)), g(rng.choice(dead_entry))
        elif p == 8:
            t[r, 2], t[r, 10] = (g(v) for v in rng.choice(dead_plain, 2, replace=False))
    assert all((pattern == p).sum() >= 50 for p in range(9))   # every kind in many rows
    for r in np.flatnonzero((t == g(y0)).any(axis=1)):          # Y0 only ever behind a pad
        assert PAD in t[r, :int(np.flatnonzero(t[r] == g(y0))[0])]
    return dict(slab=half.view(np.uint16), queries=queries, live=live, table=t, f32=False, row_base=row_base, x0=x0, y0=y0, pattern=pattern)


# ---- the visited table's probe chains ------------------------------------------------------------------------------------------------

CHAIN_N, CHAIN_DIM = 262_144, 8


def chain_rows(n=CHAIN_N):
    """The rows whose slot in the kernel's visited table (h = (row * 2654435761u) >> 19 of 8,192 slots) is one of the last two: a
    few of them fill slots 8,190 and 8,191 and every further one probes on through slot 0."""
    r = np.arange(n, dtype=np.uint64)
    h = ((r * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(19)
    return np.flatnonzero((h == 8190) | (h == 8191))


def chain_case():
    """One entry row (row 0) whose list names 16 of chain_rows(); each of those names 16 others; every other list is empty."""
    rng = np.random.default_rng(88)
    picked = chain_rows()
    half = R.unit_rows(rng, CHAIN_N, CHAIN_DIM).astype(np.float16)
    queries = R.unit_rows(rng, NQ, CHAIN_DIM)
    t = np.full((CHAIN_N, WIDTH), PAD, dtype=np.uint32)
    t[0] = rng.choice(picked, WIDTH, replace=False)
    for p in picked:
        t[p] = rng.choice(picked[picked != p], WIDTH, replace=False)
    return dict(slab=half.view(np.uint16), queries=queries, live=None, table=t, f32=False, row_base=0, picked=picked)


# ---- ties and non-finite scores ------------------------------------------------------------------------------------------------------

TIE_K_EF = ((1, 16), (16, 16), (10, 64), (256, 256))


def tie_case(identical=False):
    """16 distinct rows, each 128 times (in a seeded order): every score occurs 128 times, so every place of every answer is decided
    by the row half of the key.  identical: one row 2,048 times."""
    rng = np.random.default_rng(99)
    base = R.unit_rows(rng, 16, 64).astype(np.float16)
    half = np.tile(base[:1] if identical else base, (N if identical else N // 16, 1))[rng.permutation(N)]
    queries = R.unit_rows(rng, NQ, 64)
    live = tombstones(rng, N)
    return dict(slab=half.view(np.uint16), queries=queries, live=live, table=hand_table(rng, N, WIDTH, live), f32=False, row_base=0)


NONFINITE_CFGS = ((dict(n_entry=N_ENTRY), (10, 64)), (dict(n_entry=N_ENTRY), (16, 16)),
                  (dict(n_entry=16), (10, 256)),                             # a beam that fills step by step
                  (dict(n_entry=N_ENTRY, max_iters=3), (224, 256)))         # ~235 rows scored: never full, and -inf and NaN are in the answer


def nonfinite_case(f32):
    """Component 2 of a tenth of the rows is +inf, of a tenth -inf, of a twentieth NaN.  Queries 0-2 have a positive component 2
    (scores +inf, -inf, NaN), 3-5 a negative one (-inf, +inf, NaN), 6-8 a zero (inf x 0: NaN for all three kinds).  A step admits up
    to 64 rows — rarely a power of two — so -inf and NaN entries are sorted together with the kEmpty padding behind them."""
    rng = np.random.default_rng(111 + (1 if f32 else 0))
    half = R.unit_rows(rng, N, 64).astype(np.float16)
    queries = R.unit_rows(rng, NQ, 64)
    queries[0:3, 2] = np.abs(queries[0:3, 2]) + F32(0.05)
    queries[3:6, 2] = -np.abs(queries[3:6, 2]) - F32(0.05)
    queries[6:9, 2] = 0
    live = tombstones(rng, N)
    kind = rng.random(N)
    slab = off_f16_grid(rng, half) if f32 else half
    slab[kind < 0.10, 2] = np.inf
    slab[(kind >= 0.10) & (kind < 0.20), 2] = -np.inf
    slab[(kind >= 0.20) & (kind < 0.25), 2] = np.nan
    return dict(slab=slab if f32 else slab.view(np.uint16), queries=queries, live=live, table=hand_table(rng, N, WIDTH, live), f32=f32,
                row_base=0)


# ---- ann_ref.search with one rule broken ----------------------------------------------------------------------------------------------

MUTATIONS = ("walk past a pad", "no de-duplication within a step", "ties by row descending", "NaN above +inf")


def mutated_search(scores, live, graph, k, ef, mutation=None, n_entry=1024, degree=0, expand=4, max_iters=64, row_base=0):
    """ann_ref.search, restated with a switch per rule -> (rows, scores, count).  mutation None is ann_ref.search itself (the
    contract test holds the two equal); each of MUTATIONS breaks one rule, and a case that means to test that rule must answer
    differently under it."""
    assert mutation is None or mutation in MUTATIONS
    scores = np.ascontiguousarray(scores, dtype=F32)
    n = scores.size
    graph = np.asarray(graph, dtype=np.uint32)
    degree = int(degree) or graph.shape[1]
    alive = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    b = scores.view(np.uint32)
    ords = R.score_ord(b).astype(np.int64)
    if mutation == "NaN above +inf":
        ords[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = 1 << 32
    ords = ords.tolist()
    key = (lambda r: (-ords[r], -r)) if mutation == "ties by row descending" else (lambda r: (-ords[r], r))
    start = [e for e in R.entry_rows(n, n_entry) if alive[e]]
    visited = set(start)
    beam = sorted(start, key=key)[:ef]
    expanded = set()
    for _ in range(max_iters):
        chosen = [r for r in beam if r not in expanded][:expand]
        if not chosen:
            break
        expanded.update(chosen)
        admitted = []
        for p in chosen:
            for g in graph[p, :degree].tolist():
                if g == PAD:
                    if mutation == "walk past a pad":
                        continue
                    break
                r = g - row_base
                if r < 0 or r >= n or not alive[r] or r in visited:
                    continue
                if mutation != "no de-duplication within a step":
                    visited.add(r)
                admitted.append(r)
        visited.update(admitted)
        beam = sorted(beam + admitted, key=key)[:ef]
    count = min(k, len(beam))
    rows = np.asarray([r + row_base for r in beam[:count]], dtype=np.uint32)
    return rows, scores[np.asarray(beam[:count], dtype=np.int64)], count

"""The graph ANN search of include/fsgpu.h ("graph ANN search") as a pure function in plain Python, and the recall certificates
(recall_certificate.rs:50-292, hnsw.rs:3101-3122) restated in f64.  The per-query scores come in as a table over ALL rows — the
tests fill it from the CPU oracle's gather_dot, so every bit is the oracle's; nothing here multiplies."""
import math

import numpy as np

PAD = 0xFFFFFFFF
APPROXIMATE, UNDERFILLED, EMPTY_DESPITE_INDEXED_POINTS = 0, 1, 2


def score_ord(bits):
    """The monotone u32 image of the reference's score order (NaN as -inf, then f32::total_cmp) of f32 bit patterns."""
    b = np.asarray(bits, dtype=np.uint32).copy()
    b[(b & np.uint32(0x7FFFFFFF)) > np.uint32(0x7F800000)] = np.uint32(0xFF800000)
    neg = (b & np.uint32(0x80000000)) != 0
    return np.where(neg, ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def entry_rows(n, n_entry):
    n_entry = min(int(n_entry), int(n))
    return [i * n // n_entry for i in range(n_entry)]


def search(scores, live, graph, k, ef, n_entry=1024, degree=0, expand=4, max_iters=64, row_base=0, trace=None):
    """One query.  scores: f32 [N], the exact score of every LOCAL row; live: bool [N] or None; graph: [N, width] GLOBAL ids.
    -> (rows (global, u32), scores (f32), count, rows_scored, steps).  trace (a list) receives the beam's local rows after the entry
    phase and after every step."""
    scores = np.ascontiguousarray(scores, dtype=np.float32)
    n = scores.size
    assert 1 <= k <= ef <= 256 and 1 <= expand <= 8 and max_iters >= 1
    if n == 0:
        return np.zeros(0, np.uint32), np.zeros(0, np.float32), 0, 0, 0
    graph = np.asarray(graph, dtype=np.uint32)
    assert graph.shape[0] == n
    degree = int(degree) or graph.shape[1]
    assert degree <= graph.shape[1]
    alive = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    ords = score_ord(scores.view(np.uint32)).tolist()
    key = lambda r: (-ords[r], r)   # best first: score key descending, row ascending

    start = [e for e in entry_rows(n, n_entry) if alive[e]]
    visited = set(start)
    beam = sorted(start, key=key)[:ef]
    expanded = set()
    scored, steps = len(start), 0
    if trace is not None:
        trace.append(list(beam))
    for _ in range(max_iters):
        chosen = [r for r in beam if r not in expanded][:expand]
        if not chosen:
            break
        expanded.update(chosen)
        admitted = []
        for p in chosen:
            for g in graph[p, :degree].tolist():   # (only the lists that are walked become Python lists: tables of 2^18 rows)
                if g == PAD:
                    break
                r = g - row_base
                if r < 0 or r >= n or not alive[r] or r in visited:
                    continue
                visited.add(r)
                admitted.append(r)
        steps += 1
        scored += len(admitted)
        beam = sorted(beam + admitted, key=key)[:ef]
        if trace is not None:
            trace.append(list(beam))
    count = min(k, len(beam))
    rows = np.asarray([r + row_base for r in beam[:count]], dtype=np.uint32)
    return rows, scores[np.asarray(beam[:count], dtype=np.int64)], count, scored, steps


def flag_of(count, k, live_rows):
    """The fallback rule (hnsw.rs:299-309, 1150-1190): a count below min(k, live rows) is re-answered by the exact search."""
    if count >= min(k, live_rows):
        return APPROXIMATE
    return EMPTY_DESPITE_INDEXED_POINTS if count == 0 else UNDERFILLED


# ---- recall_certificate.rs ----------------------------------------------------------------------------------------------------------

def _finite(recalls):
    return [float(r) for r in recalls if math.isfinite(float(r))]


def _level_ok(v):
    return 0.0 <= v < 1.0   # (0.0..1.0).contains; False for a NaN


def _clamp01(v):
    return 0.0 if v < 0.0 else (1.0 if v > 1.0 else v)


def conformal_recall_lower_bound(recalls, alpha):
    if not _level_ok(alpha):
        return 0.0
    s = sorted(_finite(recalls))
    n = len(s)
    if n == 0:
        return 0.0
    rank = int(math.floor(alpha * (n + 1.0)))
    if rank == 0:
        return 0.0
    return _clamp01(s[min(rank - 1, n - 1)])


def mean_recall_lower_bound(recalls, delta):
    if not _level_ok(delta):
        return 0.0
    f = _finite(recalls)
    if not f:
        return 0.0
    n = float(len(f))
    total = 0.0
    for v in f:
        total += v
    if delta == 0.0:
        return 0.0   # ln(1 / 0) = inf: the radius is infinite
    return _clamp01(total / n - math.sqrt(math.log(1.0 / delta) / (2.0 * n)))


def mean_recall_lower_bound_bernstein(recalls, delta):
    if not _level_ok(delta) or delta == 0.0:
        return 0.0   # (delta = 0 with a constant sample is 0 x inf in the reference: outside what the tests compare)
    f = _finite(recalls)
    if len(f) < 2:
        return 0.0
    n = float(len(f))
    total = 0.0
    for v in f:
        total += v
    mean = total / n
    sq = 0.0
    for v in f:
        sq += (v - mean) * (v - mean)
    var = sq / (n - 1.0)
    ln = math.log(2.0 / delta)
    return _clamp01(mean - math.sqrt(2.0 * var * ln / n) - 7.0 * ln / (3.0 * (n - 1.0)))


def _pick(calibration, target, level, bound_fn):
    """-> (ef, bound, meets_target) or None; calibration: [(ef, recalls)]."""
    best = None
    for ef, recalls in sorted(calibration, key=lambda c: c[0]):   # stable: equal efs keep their order
        bound = bound_fn(recalls, level)
        cand = (ef, bound, bound >= target)
        if cand[2]:
            return cand
        if best is None or bound > best[1]:
            best = cand
    return best


def certified_min_ef(calibration, target, alpha):
    return _pick(calibration, target, alpha, conformal_recall_lower_bound)


def certified_min_ef_mean(calibration, target, delta):
    return _pick(calibration, target, delta, mean_recall_lower_bound_bernstein)


def calibrate(candidate_efs, measure, target, alpha):
    """calibrate_certified_ef: measure(ef) -> recalls, called in ascending ef up to the first that certifies.
    -> (chosen, sweep) of (ef, bound, meets_target), or None."""
    sweep, best = [], None
    for ef in sorted(set(int(e) for e in candidate_efs)):
        bound = conformal_recall_lower_bound(measure(ef), alpha)
        cand = (ef, bound, bound >= target)
        sweep.append(cand)
        if cand[2]:
            return cand, sweep
        if best is None or bound > best[1]:
            best = cand
    return (best, sweep) if best is not None else None


def recall_at_k_of(approx_rows, exact_rows):
    exact_rows = [int(r) for r in exact_rows]
    if not exact_rows:
        return 1.0
    have = set(int(r) for r in approx_rows)
    return sum(1 for r in exact_rows if r in have) / float(len(exact_rows))


def recall_sample(approx_rows, flag, exact_rows):
    """certified_ann_recall_sample: a flagged query counts as 0.0."""
    return 0.0 if flag else recall_at_k_of(approx_rows, exact_rows)


# ---- fixtures ------------------------------------------------------------------------------------------------------------------------

def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(np.float32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)


def knn_table(vectors_f32, m, live=None, row_base=0):
    """An [N, m] neighbour table by numpy's f32 product — near the exact one, which is all a graph has to be for these tests (the
    search is defined for ANY table).  Tombstoned rows are no targets and get an empty list."""
    x = np.ascontiguousarray(vectors_f32, dtype=np.float32)
    n = x.shape[0]
    alive = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    table = np.full((n, m), PAD, dtype=np.uint32)
    for at in range(0, n, 1024):
        s = x[at:at + 1024] @ x.T
        s[:, ~alive] = -np.inf
        s[np.arange(s.shape[0]), np.arange(at, at + s.shape[0])] = -np.inf
        take = min(m, n - 1)
        part = np.argpartition(-s, take - 1, axis=1)[:, :take]
        order = np.argsort(-np.take_along_axis(s, part, axis=1), axis=1, kind="stable")
        best = np.take_along_axis(part, order, axis=1)
        ok = np.isfinite(np.take_along_axis(s, best, axis=1))
        block = np.where(ok, best + row_base, PAD).astype(np.uint32)
        table[at:at + s.shape[0], :take] = block
    table[~alive] = PAD
    return table

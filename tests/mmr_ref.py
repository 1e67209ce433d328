"""A plain Python / numpy restatement of the reference's MMR (crates/frankensearch-fusion/src/mmr.rs:72-319), written from the Rust
source: clamped_lambda, mmr_rerank, cosine_sim, cosine_sim_pre.  Every value is an IEEE f64; numpy is used only to run the SAME
sequence of f64 operations for many pairs at once (one multiply, one add per step, in the reference's order — never a reduction
whose order numpy chooses); the fused multiply-add of the selection comes from libm."""
import ctypes
import ctypes.util
import math

import numpy as np

EPS = float(np.finfo(np.float64).eps)   # f64::EPSILON
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3


def fma(a, b, c):
    return _libm.fma(a, b, c)


def clamped_lambda(lam):
    if not math.isfinite(lam) or lam < 0.0:
        return 0.0
    return 1.0 if lam > 1.0 else lam


def cosine_sim(a, b):
    """mmr.rs:254-279: one accumulator each for the dot and both norms over the shorter length."""
    n = min(len(a), len(b))
    if n == 0:
        return 0.0
    dot = na = nb = 0.0
    for i in range(n):
        ai, bi = float(a[i]), float(b[i])
        dot += ai * bi
        na += ai * ai
        nb += bi * bi
    denom = math.sqrt(na) * math.sqrt(nb)
    if denom < EPS:
        return 0.0
    return _div(dot, denom)


def _div(x, y):
    return float(np.float64(x) / np.float64(y))   # IEEE division, NaN / inf instead of ZeroDivisionError


def root_norms(E):
    """mmr.rs:163-175 for all rows at once: norm += x * x over the elements in order, then sqrt."""
    E = np.asarray(E, dtype=np.float32).astype(np.float64)
    norm = np.zeros(E.shape[0])
    for e in range(E.shape[1]):
        norm = norm + E[:, e] * E[:, e]
    return np.sqrt(norm)


def raw_dots(E, accumulators=4):
    """The dot of cosine_sim_pre (mmr.rs:298-310) for every pair: element i goes to acc[i % 4] in ascending order,
    ((acc0 + acc1) + acc2) + acc3, then the tail.  accumulators=1 is the single-accumulator order (the tests use it to show that
    the order matters on their inputs)."""
    E = np.asarray(E, dtype=np.float32).astype(np.float64)
    n, dim = E.shape
    if accumulators == 1:
        dot = np.zeros((n, n))
        for e in range(dim):
            dot = dot + E[:, None, e] * E[None, :, e]
        return dot
    acc = [np.zeros((n, n)) for _ in range(4)]
    chunks = dim // 4
    for c in range(chunks):
        for a in range(4):
            e = c * 4 + a
            acc[a] = acc[a] + E[:, None, e] * E[None, :, e]
    dot = ((acc[0] + acc[1]) + acc[2]) + acc[3]
    for e in range(chunks * 4, dim):
        dot = dot + E[:, None, e] * E[None, :, e]
    return dot


def sim_matrix(embeddings, n):
    """sim(i, j) of mmr_rerank for the pool's first n candidates: cosine_sim_pre on a uniform pool, cosine_sim on a ragged one."""
    lens = {len(e) for e in embeddings[:n]}
    if len(lens) == 1:
        dim = lens.pop()
        if dim == 0:
            return np.zeros((n, n))
        E = np.stack([np.asarray(e, dtype=np.float32) for e in embeddings[:n]])
        root = root_norms(E)
        dot = raw_dots(E)
        denom = root[:, None] * root[None, :]
        with np.errstate(all="ignore"):
            return np.where(denom < EPS, 0.0, dot / denom)
    S = np.zeros((n, n))
    for i in range(n):
        for j in range(n):
            S[i, j] = cosine_sim(embeddings[i], embeddings[j])
    return S


def mmr_rerank(scores, embeddings, k, lam=0.7, candidate_pool=30):
    """mmr.rs:103-251.  Returns (selected indexes, the pool x pool similarity matrix)."""
    assert len(scores) == len(embeddings)
    n = min(len(scores), candidate_pool)
    if n == 0 or k == 0:
        return [], np.zeros((0, 0))
    k = min(k, n)
    lam = clamped_lambda(lam)
    diversity_weight = 1.0 - lam
    mn, mx = math.inf, -math.inf
    for s in scores[:n]:
        if math.isfinite(s):
            mn, mx = min(mn, s), max(mx, s)
    rng = mx - mn
    norm_scores = []
    for s in scores[:n]:
        s = float(s)
        if not math.isfinite(s):
            norm_scores.append(0.0)
        elif rng < EPS:
            norm_scores.append(1.0)
        else:
            with np.errstate(all="ignore"):
                norm_scores.append(float((np.float64(s) - np.float64(mn)) / np.float64(rng)))
    S = sim_matrix(embeddings, n)
    first, best = 0, -math.inf
    for i, s in enumerate(norm_scores):
        if s > best:
            first, best = i, s
    selected = [first]
    remaining = [True] * n
    remaining[first] = False
    max_sim = [-math.inf] * n
    for i in range(n):
        if remaining[i]:
            max_sim[i] = float(S[i, first])
    for _ in range(1, k):
        best_idx, best_mmr = None, -math.inf
        for i in range(n):
            if not remaining[i]:
                continue
            m = fma(lam, norm_scores[i], -(diversity_weight * max_sim[i]))
            if m > best_mmr:
                best_mmr, best_idx = m, i
        if best_idx is None:
            break
        selected.append(best_idx)
        remaining[best_idx] = False
        for i in range(n):
            if remaining[i]:
                s = float(S[i, best_idx])
                if s > max_sim[i]:
                    max_sim[i] = s
    return selected, S


def clustered(rng, n, dim, centroids=5, noise=0.35, dtype="f16"):
    """n vectors around a few centroids (so that MMR actually moves the order).  dtype "f16": unit-norm rows rounded to f16 (what an
    F16 slab holds); "f32": rows scaled over a wide dynamic range (an F32 slab, WAL vectors), where the order of the f64 additions
    shows in the bits."""
    c = rng.standard_normal((centroids, dim))
    x = c[rng.integers(0, centroids, n)] + noise * rng.standard_normal((n, dim))
    x /= np.maximum(np.linalg.norm(x, axis=1, keepdims=True), 1e-30)
    if dtype == "f16":
        return x.astype(np.float16).astype(np.float32)
    x = x * np.exp2(rng.integers(-12, 13, (1, dim))) * np.exp2(rng.integers(-3, 4, (n, 1)))
    return x.astype(np.float32)


def scores_for(rng, n, kind):
    """Relevance in rank order (descending, as a result list arrives), with ties / NaN / +-inf mixed in on request."""
    s = np.sort(rng.random(n))[::-1].copy()
    if kind == "ties" and n > 1:
        s = np.round(s * 4) / 4
    elif kind == "nonfinite" and n > 1:
        for v in (math.nan, math.inf, -math.inf):
            s[rng.integers(0, n)] = v
    elif kind == "equal":
        s[:] = 0.5
    elif kind == "negative":
        s = s - 2.0
    return s

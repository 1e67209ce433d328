"""A plain numpy restatement of the reference's query-hubness correction, written from the Rust
(crates/frankensearch-fusion/src/hubness.rs, crates/frankensearch-index/src/simd.rs:134-222, core/src/types.rs:101-133).

The dot is the reference's sequence of f32 multiplies and adds run for many (row, query) pairs at once — elementwise numpy f32
arithmetic, never a reduction whose order numpy picks.  The selection is np.sort on the total-order key; the mean is the project's
canonical order (include/fsgpu.h): v_1 >= ... >= v_k, s = v_1, s += v_2 .. v_{k-1}, (v_k + s) / k."""
import numpy as np

HREDUCE_SSE2, HREDUCE_AVX, HREDUCE_SEQ = 0, 1, 2
F32 = np.float32


def total_key(x):
    """f32::total_cmp as an unsigned key: larger key = greater.  -NaN < -inf < -0.0 < +0.0 < +inf < +NaN."""
    b = np.ascontiguousarray(x, dtype=F32).view(np.uint32)
    return np.where(b & np.uint32(0x80000000), ~b, b | np.uint32(0x80000000)).astype(np.uint32)


def key_value(k):
    k = np.ascontiguousarray(k, dtype=np.uint32)
    b = np.where(k & np.uint32(0x80000000), k & np.uint32(0x7FFFFFFF), ~k).astype(np.uint32)
    return b.view(F32)


def _hreduce(v, mode):
    """wide::f32x8::reduce_add of v[..., 8] in one of the three orders the index knows (fsgpu_index_set_hreduce)."""
    c = [v[..., i] for i in range(8)]
    if mode == HREDUCE_SEQ:
        lo = ((c[0] + c[1]) + c[2]) + c[3]
        hi = ((c[4] + c[5]) + c[6]) + c[7]
        return lo + hi
    if mode == HREDUCE_AVX:
        s0, s1, s2, s3 = c[0] + c[4], c[1] + c[5], c[2] + c[6], c[3] + c[7]
        return (s0 + s2) + (s1 + s3)
    lo = (c[0] + c[2]) + (c[1] + c[3])
    hi = (c[4] + c[6]) + (c[5] + c[7])
    return lo + hi


def dot_many(x, y, hreduce=HREDUCE_SSE2):
    """dot_product_f32_f32 of every row of x [n, d] with every row of y [m, d] -> [n, m] f32."""
    x = np.ascontiguousarray(x, dtype=F32)
    y = np.ascontiguousarray(y, dtype=F32)
    n, d = x.shape
    m = y.shape[0]
    groups, chunks = d // 32, d // 8
    with np.errstate(all="ignore"):
        acc = [np.zeros((n, m, 8), F32) for _ in range(4)]
        for g in range(groups):
            for a in range(4):
                o = 32 * g + 8 * a
                p = x[:, None, o:o + 8] * y[None, :, o:o + 8]     # a multiply ...
                acc[a] = acc[a] + p                               # ... and an add, no fma
        v = (acc[0] + acc[1]) + (acc[2] + acc[3])
        for c in range(4 * groups, chunks):                       # leftover chunks join AFTER the tree
            v = v + x[:, None, 8 * c:8 * c + 8] * y[None, :, 8 * c:8 * c + 8]
        r = _hreduce(v, hreduce)
        for i in range(8 * chunks, d):                            # unfused tail
            p = x[:, None, i] * y[None, :, i]
            r = r + p
    return r.astype(F32)


def canonical_mean(top_desc):
    """top_desc [n, k] f32, greatest first under total_cmp -> [n] f32 in the canonical order."""
    top_desc = np.ascontiguousarray(top_desc, dtype=F32)
    k = top_desc.shape[1]
    with np.errstate(all="ignore"):
        if k == 1:
            return (top_desc[:, 0] / F32(1.0)).astype(F32)
        s = top_desc[:, 0].copy()
        for i in range(1, k - 1):
            s = s + top_desc[:, i]
        return ((top_desc[:, k - 1] + s) / F32(k)).astype(F32)


def select_top(sims, k):
    """sims [n, Q] -> the k greatest per row under total_cmp, greatest first, [n, k]."""
    keys = np.sort(total_key(sims), axis=1)[:, ::-1][:, :k]
    return key_value(np.ascontiguousarray(keys))


def compute_query_hubness(docs, queries, kq, hreduce=HREDUCE_SSE2, want_topk=False, block=256):
    """docs [n, d], queries [Q, d] (equal lengths; ragged inputs go through compute_query_hubness_ragged)."""
    docs = np.ascontiguousarray(docs, dtype=F32)
    n = docs.shape[0]
    queries = np.ascontiguousarray(queries, dtype=F32)
    nq = queries.shape[0] if queries.ndim == 2 else 0
    if nq == 0 or kq == 0:
        return (np.zeros(n, F32), np.zeros((n, 0), F32)) if want_topk else np.zeros(n, F32)
    k = min(kq, nq)
    out = np.zeros(n, F32)
    tops = np.zeros((n, k), F32)
    for r0 in range(0, n, block):
        top = select_top(dot_many(docs[r0:r0 + block], queries, hreduce), k)
        tops[r0:r0 + block] = top
        out[r0:r0 + block] = canonical_mean(top)
    return (out, tops) if want_topk else out


def compute_query_hubness_ragged(docs, queries, kq, hreduce=HREDUCE_SSE2):
    """Lists of vectors of any lengths: every dot runs over the common prefix (hubness.rs:157-161)."""
    if len(queries) == 0 or kq == 0:
        return np.zeros(len(docs), F32)
    k = min(kq, len(queries))
    out = np.zeros(len(docs), F32)
    for i, d in enumerate(docs):
        d = np.asarray(d, F32)
        sims = []
        for q in queries:
            q = np.asarray(q, F32)
            n = min(d.size, q.size)
            sims.append(dot_many(d[None, :n], q[None, :n], hreduce)[0, 0] if n else F32(0.0))
        out[i] = canonical_mean(select_top(np.asarray(sims, F32)[None, :], k))[0]
    return out


def rank_score_key(score):
    """VectorHit::cmp_by_score: NaN as -inf, then total_cmp (types.rs:101-115)."""
    s = F32(score)
    if np.isnan(s):
        s = F32(-np.inf)
    return int(total_key(np.asarray([s], F32))[0])


def apply_hubness_penalty(hits, table, beta, resort=True):
    """hits: (doc_id, score, index).  hubness.rs:67-86, then the sort of correct_phase1_pool by cmp_rank (stable)."""
    beta = F32(beta)
    hits = [(d, F32(s), int(i)) for d, s, i in hits]
    if not np.isfinite(beta) or beta <= 0:
        return hits
    table = np.asarray(table, F32).reshape(-1)
    out = []
    with np.errstate(all="ignore"):
        for d, s, i in hits:
            r = table[i] if i < table.size else F32(0.0)
            p = F32(beta * r)
            out.append((d, F32(s - p), i))
    if resort:
        out.sort(key=lambda h: (-rank_score_key(h[1]), h[0].encode()))
    return out


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F32)

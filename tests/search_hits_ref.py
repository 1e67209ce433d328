"""numpy restatement of what fsgpu_search_hits_batched computes, written from the semantics alone:

  * dot_f32_f32: the WAL score in the three horizontal-reduce orders (f32 arithmetic step by step, no fused multiply-add);
  * class_tables: the doc-id class of every main row and WAL entry and the shadowed main rows;
  * search_hits: merge of a best-first main list with the WAL scores, the first k, then the three drops, on doc-id strings;
  * resolve_by_class: the same drops on class numbers, the way the device does them.

tests/test_search_hits_contract.py pins it against the oracle on the CPU; tests/test_gpu_search_hits_batched.py uses it for the WAL
kernel's bits."""
import numpy as np

F32 = np.float32
HREDUCE_SSE2, HREDUCE_AVX, HREDUCE_SEQ = 0, 1, 2


def wal_scores_modes(wal, q):
    """{hreduce: scores [W]} of every row of wal [W, n] against q [n], for the three horizontal-add orders: groups of 32 into four
    8-lane accumulators, (a0 + a1) + (a2 + a3), the leftover chunks of 8 into that sum, the horizontal add, then the last n % 8
    products one by one."""
    wal = np.ascontiguousarray(wal, dtype=F32)
    q = np.ascontiguousarray(q, dtype=F32)
    W, n = wal.shape
    groups, chunks = n // 32, n // 8
    with np.errstate(over="ignore", invalid="ignore"):
        p = wal * q[None, :]                                   # every product rounded to f32 once
        acc = np.zeros((W, 4, 8), F32)
        for g in range(groups):
            acc = acc + p[:, 32 * g:32 * g + 32].reshape(W, 4, 8)
        v = (acc[:, 0] + acc[:, 1]) + (acc[:, 2] + acc[:, 3])  # [W, 8]
        for c in range(4 * groups, chunks):
            v = v + p[:, 8 * c:8 * c + 8]
        out = {}
        for hreduce in (HREDUCE_SSE2, HREDUCE_AVX, HREDUCE_SEQ):
            if hreduce == HREDUCE_SEQ:
                lo = ((v[:, 0] + v[:, 1]) + v[:, 2]) + v[:, 3]
                hi = ((v[:, 4] + v[:, 5]) + v[:, 6]) + v[:, 7]
            elif hreduce == HREDUCE_AVX:
                s0, s1, s2, s3 = v[:, 0] + v[:, 4], v[:, 1] + v[:, 5], v[:, 2] + v[:, 6], v[:, 3] + v[:, 7]
                lo, hi = s0 + s2, s1 + s3
            else:
                lo = (v[:, 0] + v[:, 2]) + (v[:, 1] + v[:, 3])
                hi = (v[:, 4] + v[:, 6]) + (v[:, 5] + v[:, 7])
            r = lo + hi
            for i in range(8 * chunks, n):
                r = r + p[:, i]
            assert r.dtype == F32
            out[hreduce] = r
    return out


def wal_scores(wal, q, hreduce=HREDUCE_SSE2):
    return wal_scores_modes(wal, q)[hreduce]


def dot_f32_f32(a, b, hreduce=HREDUCE_SSE2):
    return wal_scores(np.asarray(a, F32)[None, :], b, hreduce)[0]


def score_ord(score):
    """Larger = ranks earlier: NaN counts as -inf, then the total order of the f32 bit patterns (-0.0 below +0.0)."""
    bits = int(np.asarray(score, F32).view(np.uint32))
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        bits = 0xFF800000
    return (~bits & 0xFFFFFFFF) if bits & 0x80000000 else (bits | 0x80000000)


def class_tables(main_ids, wal_ids):
    """(main_class [N], wal_class [W], shadowed [N] bool).  Equal ids <=> equal classes: a main row's class is the first main row with
    its id; a WAL entry's is that of the main row with its id (live or not), else N + the first WAL index with the id."""
    n = len(main_ids)
    first_main, main_class = {}, np.empty(n, np.uint32)
    for r, d in enumerate(main_ids):
        main_class[r] = first_main.setdefault(d, r)
    first_wal, wal_class = {}, np.empty(len(wal_ids), np.uint32)
    for w, d in enumerate(wal_ids):
        wal_class[w] = first_main[d] if d in first_main else first_wal.setdefault(d, n + w)
    in_wal = set(wal_ids)
    shadowed = np.array([d in in_wal for d in main_ids], bool)
    return main_class, wal_class, shadowed


def merge_first_k(main_hits, wal_sc, nrows, k):
    """main_hits: [(row, score)] best first; wal_sc [W].  -> the first k of both under (score order desc, index asc), a WAL entry's
    index being nrows + its WAL index (behind every main row); non-finite WAL scores are skipped."""
    cand = [(int(r), F32(s)) for r, s in main_hits]
    cand += [(nrows + w, F32(s)) for w, s in enumerate(wal_sc) if np.isfinite(s)]
    cand.sort(key=lambda c: (-score_ord(c[1]), c[0]))
    return cand[:k]


def search_hits(main_hits, wal_sc, live, main_ids, wal_ids, k):
    """The semantics on doc-id strings -> [(row, score)].  live: bool [N] or None."""
    nrows = len(main_ids)
    in_wal, seen, out = set(wal_ids), set(), []
    for row, s in merge_first_k(main_hits, wal_sc, nrows, k):
        if row < nrows:
            if live is not None and not live[row]:
                continue
            if main_ids[row] in in_wal:
                continue
            d = main_ids[row]
        else:
            d = wal_ids[row - nrows]
        if d in seen:
            continue
        seen.add(d)
        out.append((row, s))
    return out


def resolve_by_class(first_k, live, main_class, wal_class, shadowed, nrows):
    """The drops on class numbers (what resolve_hits_kernel does): an entry that is live and not shadowed is emitted iff no earlier
    such entry has its class."""
    kept, out = [], []
    for row, s in first_k:
        if row < nrows:
            if (live is not None and not live[row]) or shadowed[row]:
                continue
            c = int(main_class[row])
        else:
            c = int(wal_class[row - nrows])
        if c in kept:
            continue
        kept.append(c)
        out.append((row, s))
    return out

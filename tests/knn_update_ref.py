"""The contract of fsgpu_index_update_knn_graph (include/fsgpu.h) restated in plain numpy: the packed total order, the
classes of a current row, the update itself and a brute-force build to compare it with.

Scores never come from numpy: `search(x, k)` is the exact row-level top-k of the query "row x widened to f32" (local rows, scores)
and `score(x, targets)` the scores of the given target rows for that query — the tests hand in the CPU oracle's functions, so the
bits are dot_product_f16_bytes_f32 / dot_product_f32_bytes_f32 in the chosen hreduce order.  Everything here stays memory-safe on a
hostile old table: every id is a Python int that is range-checked before it indexes anything.

`mutate` switches ONE rule off, for the tests that show each rule is load-bearing:
  "dropped_stays_clean"       a row that lists a dropped row keeps its (shortened) list instead of being searched again
  "ties_row_desc"             equal keys order by row descending
  "resurrected_not_added"     a live row whose predecessor's list is empty is kept-clean, not added
  "nonmonotone_keeps_clean"   a map that is not monotone does not make the kept rows dirty
  "plain_dot"                 (the caller's: hand in a `score` that sums left to right)
"""
import numpy as np

F32 = np.float32
PAD = 0xFFFFFFFF
DEAD, ADDED, CLEAN, DIRTY = 0, 1, 2, 3


def score_ord(bits: int) -> int:
    """The monotone u32 image of key(score): NaN ranks as -inf, then f32::total_cmp (-0.0 < +0.0)."""
    bits = int(bits) & 0xFFFFFFFF
    if (bits & 0x7FFFFFFF) > 0x7F800000:
        bits = 0xFF800000
    return (~bits) & 0xFFFFFFFF if bits & 0x80000000 else bits | 0x80000000


def sortkey(bits: int, row: int) -> int:
    """Greater = better: key(score) descending, then row ascending; distinct for distinct rows."""
    return (score_ord(bits) << 32) | ((~int(row)) & 0xFFFFFFFF)


def order(entries, mutate=None):
    """entries: (score bits, row) pairs -> best first under the total order."""
    if mutate == "ties_row_desc":
        return sorted(entries, key=lambda e: (-score_ord(e[0]), -int(e[1])))
    return sorted(entries, key=lambda e: -sortkey(e[0], e[1]))


def bits_of(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def list_from_topk(hit_rows, hit_scores, self_row, m):
    """The self rule of the build: the top-(m + 1) with the self entry taken out, else the last entry dropped -> (rows, score bits)."""
    rows = [int(r) for r in hit_rows][: m + 1]
    sc = [int(b) for b in bits_of(hit_scores)][: m + 1]
    if self_row in rows:
        at = rows.index(self_row)
        del rows[at], sc[at]
    elif len(rows) == m + 1:
        rows.pop(), sc.pop()
    return rows, sc


def _write(rows_out, sims_out, x, rows, sc, row_base):
    for c, (r, b) in enumerate(zip(rows, sc)):
        rows_out[x, c] = (r + row_base) & 0xFFFFFFFF
        sims_out[x, c] = b


def build(search, n, live, m, row_base=0, sources=None):
    """Brute force: ([n, m] global rows, [n, m] sim BITS as uint32) of fsgpu_index_build_knn_graph; `sources` limits the rows that
    are computed (the others stay padding)."""
    rows_out = np.full((n, m), PAD, dtype=np.uint32)
    sims_out = np.zeros((n, m), dtype=np.uint32)
    for x in (range(n) if sources is None else sources):
        x = int(x)
        if not live[x]:
            continue
        hr, hs = search(x, m + 1)
        rows, sc = list_from_topk(hr, hs, x, m)
        _write(rows_out, sims_out, x, rows, sc, row_base)
    return rows_out, sims_out


def classify(old_rows, old_sim_bits, old_row_base, new_to_old, live, n, mutate=None):
    """-> (cls uint8 [n], mapped: {x: [(bits, current row)]} for kept rows with their surviving entries, monotone)."""
    old_rows = np.asarray(old_rows)
    old_len, m = old_rows.shape
    n2o = [int(p) for p in (range(n) if new_to_old is None else new_to_old)]
    n2o = [p if p < old_len else PAD for p in n2o] if new_to_old is None else n2o
    inv = {}
    monotone, prev = True, -1
    for x, p in enumerate(n2o):
        if p == PAD or p >= old_len:
            continue
        inv[p] = x
        if p <= prev:
            monotone = False
        prev = p
    if mutate == "nonmonotone_keeps_clean":
        monotone = True
    cls = np.zeros(n, dtype=np.uint8)
    mapped = {}
    for x in range(n):
        if not live[x]:
            cls[x] = DEAD
            continue
        p = n2o[x]
        lst = [] if (p == PAD or p >= old_len) else [int(v) for v in old_rows[p]]
        length = lst.index(PAD) if PAD in lst else len(lst)       # the list ends at its first pad
        if length == 0:
            if mutate == "resurrected_not_added" and p != PAD and p < old_len:
                cls[x], mapped[x] = CLEAN, []
            else:
                cls[x] = ADDED
            continue
        kept, dropped = [], False
        for c in range(length):
            o = lst[c] - old_row_base
            y = inv.get(o, PAD) if 0 <= o < old_len else PAD
            if y == PAD or y >= n or not live[y]:
                dropped = True
            else:
                kept.append((int(old_sim_bits[p, c]), y))
        if mutate == "dropped_stays_clean":
            dropped = False
        cls[x] = DIRTY if (dropped or not monotone) else CLEAN
        mapped[x] = kept
    return cls, mapped, monotone


def update(old_rows, old_sims, new_to_old, live, n, search, score, old_row_base=0, row_base=0, max_added_fraction=1.0,
           join_covers=True, mutate=None, sources=None):
    """-> ([n, m] global rows, [n, m] sim bits, stats).  `sources`: compute only these rows' lists (stats and classes are whole)."""
    old_rows = np.asarray(old_rows, dtype=np.uint32)
    old_bits = bits_of(old_sims).reshape(old_rows.shape)
    m = old_rows.shape[1]
    cls, mapped, monotone = classify(old_rows, old_bits, old_row_base, new_to_old, live, n, mutate)
    added = [int(x) for x in np.flatnonzero(cls == ADDED)]
    st = {"rows": n, "dead": int((cls == DEAD).sum()), "added": len(added), "kept_clean": int((cls == CLEAN).sum()),
          "kept_dirty": int((cls == DIRTY).sum())}
    st["rebuilt"] = 1 if not monotone else 3 if not join_covers else 2 if float(len(added)) > float(F32(max_added_fraction)) * float(n) else 0
    rebuilt = st["rebuilt"] != 0
    st["searched_sources"] = n - st["dead"] if rebuilt else st["added"] + st["kept_dirty"]
    st["join_pairs"] = 0 if rebuilt else st["kept_clean"] * st["added"]
    rows_out = np.full((n, m), PAD, dtype=np.uint32)
    sims_out = np.zeros((n, m), dtype=np.uint32)
    added_arr = np.asarray(added, dtype=np.uint32)
    for x in (range(n) if sources is None else sources):
        x = int(x)
        if cls[x] == DEAD:
            continue
        if rebuilt or cls[x] != CLEAN:
            hr, hs = search(x, m + 1)
            rows, sc = list_from_topk(hr, hs, x, m)
        else:
            entries = list(mapped[x])
            if added:
                entries += list(zip((int(b) for b in bits_of(score(x, added_arr))), added))
            best = order(entries, mutate)[:m]
            rows, sc = [e[1] for e in best], [e[0] for e in best]
        _write(rows_out, sims_out, x, rows, sc, row_base)
    if sources is None:
        is_added = np.zeros(n + 1, dtype=bool)
        is_added[added] = True
        local = np.where(rows_out == PAD, n, (rows_out.astype(np.int64) - row_base).clip(0, n))
        st["join_entries"] = int(is_added[local][cls == CLEAN].sum())
    return rows_out, sims_out, st


def join(work_rows, work_bits, cls, added_rows, score, m, mutate=None):
    """One launch of the join alone: every kept-clean row's list merged with one block of added rows; other rows untouched."""
    rows_out, bits_out = np.array(work_rows, dtype=np.uint32), np.array(work_bits, dtype=np.uint32)
    added = [int(a) for a in added_rows]
    for x in np.flatnonzero(np.asarray(cls) == CLEAN):
        x = int(x)
        entries = [(int(b), int(r)) for r, b in zip(rows_out[x], bits_out[x]) if int(r) != PAD]
        entries += list(zip((int(b) for b in bits_of(score(x, np.asarray(added, dtype=np.uint32)))), added))
        best = order(entries, mutate)[:m]
        rows_out[x], bits_out[x] = PAD, 0
        for c, (b, r) in enumerate(best):
            rows_out[x, c], bits_out[x, c] = r, b
    return rows_out, bits_out

"""The contract of fsgpu_index_update_knn_graph without a GPU: knn_update_ref.update over the table of the index as it was equals the
brute-force build of the index as it is, byte for byte, with every score from the CPU oracle's exact dot; every rule of the contract
is shown to be load-bearing by a mutation; the reference stays memory-safe and deterministic on a hostile old table."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import knn_update_ref as U  # noqa: E402

F32 = np.float32
PAD = U.PAD


def unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float16)


def fns(oracle, vec, live, mode=0):
    """(search, score) over an f16 corpus: the oracle's exact top-k and its dot of chosen rows, query = the row widened."""
    slab, wide = np.ascontiguousarray(vec).view(np.uint16), vec.astype(F32)
    live = np.asarray(live, dtype=bool)

    def search(x, k):
        return oracle.search_top_k(slab, wide[x], k, live=live, hreduce=mode)

    def score(x, rows):
        return oracle.gather_dot(slab, wide[x], np.asarray(rows, dtype=np.uint32), hreduce=mode)

    return search, score


def rewrite(rng, vec0, live0, drop=(), add=None, front=False, back=False):
    """E1 from E0 as a compaction or a vacuum makes it: the old rows not in `drop` in their order, the rows of `add` inserted at
    seeded places (front / back: all before / all after the old rows) -> (vec1, live1, new_to_old)."""
    keep = [r for r in range(len(vec0)) if r not in set(int(d) for d in drop)]
    n_add = 0 if add is None else len(add)
    slots = ["old"] * len(keep) + ["new"] * n_add
    if not front and not back:
        slots = [slots[i] for i in rng.permutation(len(slots))]
    elif front:
        slots = ["new"] * n_add + ["old"] * len(keep)
    vec1, live1, n2o, ko, ka = [], [], [], 0, 0
    for s in slots:
        if s == "old":
            vec1.append(vec0[keep[ko]]), live1.append(bool(live0[keep[ko]])), n2o.append(keep[ko])
            ko += 1
        else:
            vec1.append(add[ka]), live1.append(True), n2o.append(PAD)
            ka += 1
    return np.stack(vec1), np.array(live1, dtype=bool), np.array(n2o, dtype=np.uint32)


def old_table(oracle, vec0, live0, m, mode=0):
    search, _ = fns(oracle, vec0, live0, mode)
    rows, bits = U.build(search, len(vec0), live0, m)
    return rows, bits.view(F32)


def check(oracle, vec0, live0, vec1, live1, n2o, m, mode=0, mutate=None, score=None, **kw):
    """update(build(E0), map) against build(E1) -> (equal?, update's stats)."""
    old_rows, old_sims = old_table(oracle, vec0, live0, m, mode)
    search, exact = fns(oracle, vec1, live1, mode)
    got_r, got_b, st = U.update(old_rows, old_sims, n2o, live1, len(vec1), search, score or exact, mutate=mutate, **kw)
    want_r, want_b = U.build(search, len(vec1), live1, m)
    return bool((got_r == want_r).all() and (got_b == want_b).all()), st


CORPORA = [(40, 8), (131, 43), (400, 72), (97, 64)]


@pytest.mark.parametrize("n,dim", CORPORA)
@pytest.mark.parametrize("what", ["deletes", "additions", "both"])
def test_update_equals_build_for_deletes_additions_and_both(oracle, n, dim, what):
    rng = np.random.default_rng(n * 1000 + dim)
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    drop = rng.choice(n, size=max(n // 30, 1), replace=False) if what != "additions" else ()
    add = unit_rows(rng, max(n // 50, 2), dim) if what != "deletes" else None
    vec1, live1, n2o = rewrite(rng, vec0, live0, drop, add)
    for mode in (0, 1, 2):
        same, st = check(oracle, vec0, live0, vec1, live1, n2o, 10, mode)
        assert same, (what, mode, st)
        assert st["rebuilt"] == 0 and st["searched_sources"] == st["added"] + st["kept_dirty"]
        assert st["kept_clean"] > 0 and (what == "additions" or st["kept_dirty"] > 0) and (what == "deletes") == (st["added"] == 0)


def test_soft_deletes_and_resurrected_rows_under_the_identity_map(oracle):
    rng = np.random.default_rng(7)
    n, dim, m = 150, 43, 10
    vec = unit_rows(rng, n, dim)
    live0 = np.ones(n, dtype=bool)
    live0[[3, 77, 149]] = False
    live1 = live0.copy()
    live1[[3, 149]] = True               # brought back: their old lists are empty, so they are added rows
    live1[[10, 11, 90]] = False          # and three soft deletes
    same, st = check(oracle, vec, live0, vec, live1, None, m)
    assert same and st["added"] == 2 and st["dead"] == 4 and st["kept_dirty"] > 0 and st["kept_clean"] > 0
    same, _ = check(oracle, vec, live0, vec, live1, None, m, mutate="resurrected_not_added")
    assert not same, "a resurrected row that is not treated as added went unnoticed"


def test_a_corpus_that_grows_from_5_rows_to_12_at_m_10(oracle):
    rng = np.random.default_rng(12)
    vec0, live0 = unit_rows(rng, 5, 24), np.ones(5, dtype=bool)
    vec1, live1, n2o = rewrite(rng, vec0, live0, (), unit_rows(rng, 7, 24))
    same, st = check(oracle, vec0, live0, vec1, live1, n2o, 10)
    # (a kept row has 4 old entries and 7 candidates for 10 places: six or seven of the added rows enter each list)
    assert same and st["added"] == 7 and st["kept_clean"] == 5 and 30 <= st["join_entries"] <= 35
    # ... and from ONE row: its old list is empty, so every row is added
    vec1, live1, n2o = rewrite(rng, vec0[:1], live0[:1], (), unit_rows(rng, 4, 24))
    same, st = check(oracle, vec0[:1], live0[:1], vec1, live1, n2o, 10)
    assert same and st["added"] == 5 and st["kept_clean"] == 0


def _tie_corpus(rng, n, dim, pairs):
    vec = unit_rows(rng, n, dim)
    twins = vec[rng.choice(n, size=pairs, replace=False)].copy()
    return vec, twins


@pytest.mark.parametrize("front", [True, False])
def test_an_added_row_that_ties_with_the_mth_entry_enters_only_with_the_lower_id(oracle, front):
    rng = np.random.default_rng(33)
    n, dim, m = 80, 16, 3
    vec0, twins = _tie_corpus(rng, n, dim, 8)          # the added rows are bit copies of eight old rows
    live0 = np.ones(n, dtype=bool)
    vec1, live1, n2o = rewrite(rng, vec0, live0, (), twins, front=front, back=not front)
    old_rows, old_sims = old_table(oracle, vec0, live0, m)
    search, score = fns(oracle, vec1, live1)
    got_r, got_b, st = U.update(old_rows, old_sims, n2o, live1, len(vec1), search, score)
    want_r, want_b = U.build(search, len(vec1), live1, m)
    assert (got_r == want_r).all() and (got_b == want_b).all() and st["kept_dirty"] == 0
    # witnesses: a kept list whose LAST entry ties with an added twin
    added = set(np.flatnonzero(n2o == PAD).tolist())
    inv = {int(p): x for x, p in enumerate(n2o) if p != PAD}
    entered = stayed_out = 0
    for x in range(len(vec1)):
        if x in added:
            continue
        old_last = inv[int(old_rows[n2o[x], m - 1])]
        tie = [a for a in added if np.array_equal(vec1[a], vec1[old_last]) and a != x]
        if not tie:
            continue
        if tie[0] < old_last:
            entered += int(got_r[x, m - 1] == tie[0] and old_last not in got_r[x].tolist() and got_b[x, m - 1] == U.bits_of(old_sims)[n2o[x], m - 1])
        else:
            stayed_out += int(got_r[x, m - 1] == old_last and tie[0] not in got_r[x].tolist())
    assert (entered if front else stayed_out) > 0, "no list of this corpus has the tie at its m-th place"
    same, _ = check(oracle, vec0, live0, vec1, live1, n2o, m, mutate="ties_row_desc")
    assert not same, "ties broken by row descending went unnoticed"


def test_nan_and_infinite_scores_from_planted_rows(oracle):
    rng = np.random.default_rng(99)
    n, dim, m = 120, 43, 10
    vec0 = unit_rows(rng, n, dim)
    vec0[5, 0], vec0[6, 1], vec0[7, 2] = np.float16(np.inf), np.float16(-np.inf), np.float16(np.nan)
    vec0[8, :2] = [np.float16(np.inf), np.float16(-np.inf)]       # inf - inf inside one dot
    live0 = np.ones(n, dtype=bool)
    add = unit_rows(rng, 5, dim)
    add[0, 0], add[1, 40], add[2, 42] = np.float16(np.inf), np.float16(np.nan), np.float16(-np.inf)   # group, leftover, tail
    vec1, live1, n2o = rewrite(rng, vec0, live0, [20, 21], add)
    for mode in (0, 2):
        same, st = check(oracle, vec0, live0, vec1, live1, n2o, m, mode)
        assert same, (mode, st)


def test_a_map_that_is_not_monotone_is_a_rebuild_and_still_exact(oracle):
    rng = np.random.default_rng(5)
    n, dim, m = 90, 16, 3
    vec0, twins = _tie_corpus(rng, n, dim, 10)
    vec0[rng.choice(n, size=10, replace=False)] = twins          # ten pairs of duplicate rows inside E0
    live0 = np.ones(n, dtype=bool)
    n2o = np.arange(n, dtype=np.uint32)[::-1].copy()             # every tie now breaks the other way
    vec1, live1 = vec0[::-1].copy(), live0.copy()
    same, st = check(oracle, vec0, live0, vec1, live1, n2o, m)
    assert same and st["rebuilt"] == 1 and st["kept_clean"] == 0 and st["searched_sources"] == n and st["join_pairs"] == 0
    same, st = check(oracle, vec0, live0, vec1, live1, n2o, m, mutate="nonmonotone_keeps_clean")
    assert not same and st["rebuilt"] == 0, "kept-clean rows under a map that is not monotone went unnoticed"


def test_a_row_that_lists_a_dropped_row_must_not_stay_clean(oracle):
    rng = np.random.default_rng(21)
    n, dim = 131, 43
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    vec1, live1, n2o = rewrite(rng, vec0, live0, rng.choice(n, size=5, replace=False), None)
    same, _ = check(oracle, vec0, live0, vec1, live1, n2o, 10, mutate="dropped_stays_clean")
    assert not same


@pytest.mark.parametrize("dim", [43, 72])
def test_the_join_must_score_in_the_byte_dots_order_not_left_to_right(oracle, dim):
    """dim 43: one group, one leftover chunk, a tail of three; dim 72: two groups and a leftover chunk."""
    rng = np.random.default_rng(dim)
    n, m = 200, 10
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    vec1, live1, n2o = rewrite(rng, vec0, live0, (), unit_rows(rng, 12, dim))
    wide = vec1.astype(F32)

    def plain(x, rows):
        out = np.zeros(len(rows), dtype=F32)
        for i, r in enumerate(rows):
            s = F32(0)
            for e in range(dim):
                s = F32(s + F32(wide[x, e] * wide[int(r), e]))
            out[i] = s
        return out

    same, _ = check(oracle, vec0, live0, vec1, live1, n2o, m)
    assert same
    same, _ = check(oracle, vec0, live0, vec1, live1, n2o, m, score=plain)
    assert not same, "a left-to-right dot in the join went unnoticed"


def test_the_fallbacks_report_themselves_and_are_the_same_table(oracle):
    rng = np.random.default_rng(3)
    n, dim = 97, 64
    vec0, live0 = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    vec1, live1, n2o = rewrite(rng, vec0, live0, [4], unit_rows(rng, 3, dim))
    same, st = check(oracle, vec0, live0, vec1, live1, n2o, 10, max_added_fraction=0.0)
    assert same and st["rebuilt"] == 2 and st["searched_sources"] == len(vec1) and st["join_pairs"] == 0
    same, st = check(oracle, vec0, live0, vec1, live1, n2o, 10, join_covers=False)
    assert same and st["rebuilt"] == 3


def test_the_reference_is_memory_safe_and_deterministic_on_a_hostile_old_table(oracle):
    rng = np.random.default_rng(666)
    n, dim, m = 60, 8, 6
    vec, live = unit_rows(rng, n, dim), np.ones(n, dtype=bool)
    live[[9, 30]] = False
    old_len = 50
    old_rows = rng.integers(0, 2**32, size=(old_len, m), dtype=np.uint64).astype(np.uint32)      # ids out of range
    old_rows[::3] = rng.integers(0, old_len, size=old_rows[::3].shape).astype(np.uint32) + 7     # in range of old_row_base 7
    old_rows[1::4, 2] = PAD                                                                      # pads in mid-list
    for r in range(0, old_len, 5):
        old_rows[r, 0] = r + 7                                                                   # self-loops
        old_rows[r, 1] = old_rows[r, 3] = (r + 1) % old_len + 7                                  # repeated ids
    old_sims = rng.standard_normal((old_len, m)).astype(F32)
    old_sims[2, 0] = np.nan
    n2o = np.full(n, PAD, dtype=np.uint32)
    n2o[rng.choice(n, size=40, replace=False)] = rng.choice(old_len, size=40, replace=False).astype(np.uint32)   # not monotone either
    search, score = fns(oracle, vec, live)
    for keep_clean in (None, "nonmonotone_keeps_clean"):
        a = U.update(old_rows, old_sims, n2o, live, n, search, score, old_row_base=7, row_base=1000, mutate=keep_clean)
        b = U.update(old_rows.copy(), old_sims.copy(), n2o.copy(), live, n, search, score, old_row_base=7, row_base=1000, mutate=keep_clean)
        assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
        real = a[0][a[0] != PAD]
        assert ((real >= 1000) & (real < 1000 + n)).all()
        assert (a[0][~live] == PAD).all()
    with pytest.raises(Exception):
        U.order([(0, 1), "not an entry"])


def test_the_packed_total_order():
    b = lambda x: int(np.array([x], dtype=F32).view(np.uint32)[0])
    nan, ninf = b(np.nan), b(-np.inf)
    best_first = U.order([(b(-0.0), 4), (b(0.0), 9), (nan, 3), (ninf, 2), (b(1.0), 7), (b(1.0), 5), (b(np.inf), 8), (nan | 0x80000000, 1)])
    assert [r for _, r in best_first] == [8, 5, 7, 9, 4, 1, 2, 3]      # NaN of either sign ranks as -inf; ties by row ascending
    assert U.sortkey(ninf, 0xFFFFFFFE) > (U.score_ord(ninf) << 32)     # a real entry beats the pad's key

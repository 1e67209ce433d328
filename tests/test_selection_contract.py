"""tests/selection_ref.py against brute force (a Python sort with an explicit comparator, f32 comparisons spelled out), and its restated
launcher predicates against fsgpu_lab_select_check.  No GPU: the check looks at its arguments before it looks for a device."""
import functools
import math
import struct

import numpy as np
import pytest

import selection_ref as R

SPECIALS = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0, -1.5, -1.5, 2.0, 2.0, 2.0, -3.25, 1e-40, -1e-40]


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    build()


def bits_of(x):
    return struct.unpack("<I", struct.pack("<f", x))[0]


def total_cmp(a_bits, b_bits):
    """f32::total_cmp on bit patterns with NaN ranked as -inf: -1, 0, 1 — written with float comparisons and the sign of zero, not with
    selection_ref's integer image."""
    def val(bits):
        f = struct.unpack("<f", struct.pack("<I", bits))[0]
        return float("-inf") if f != f else f
    a, b = val(a_bits), val(b_bits)
    if a < b:
        return -1
    if a > b:
        return 1
    if a == 0.0 and b == 0.0:   # -0.0 ranks below +0.0
        sa, sb = math.copysign(1.0, a), math.copysign(1.0, b)
        return -1 if sa < sb else (1 if sa > sb else 0)
    return 0


def before(x, y):
    """cmp for sorted(): x ranks before y iff its score is greater, or equal with the lower row."""
    c = total_cmp(R.score_bits(x), R.score_bits(y))
    if c:
        return -c
    return -1 if R.row_of(x) < R.row_of(y) else (1 if R.row_of(x) > R.row_of(y) else 0)


def brute_best_first(entries):
    return sorted((int(e) for e in entries if int(e) != R.KEMPTY), key=functools.cmp_to_key(before))


def random_entries(rng, n, holes=0.2):
    scores = np.where(rng.random(n) < 0.5, rng.choice(np.array(SPECIALS, np.float32), n), rng.standard_normal(n).astype(np.float32)).astype(np.float32)
    e = R.pack(scores, rng.permutation(4 * n)[:n].astype(np.uint64))
    e[rng.random(n) < holes] = np.uint64(R.KEMPTY)
    return e


@pytest.mark.parametrize("seed", range(8))
def test_order_matches_brute_force(seed):
    rng = np.random.default_rng(seed)
    e = random_entries(rng, 60)
    assert R.best_first(e) == brute_best_first(e)
    # (negative NaN, the NaN with a payload and -inf all rank together, by row)
    odd = [int(R.pack(np.float32(0), r)) & 0xFFFFFFFF | (b << 32) for r, b in enumerate((0xFFC00001, 0x7FC00000, 0xFF800000, 0x7F800001))]
    assert R.best_first(odd) == sorted(odd, key=R.row_of) == brute_best_first(odd)


@pytest.mark.parametrize("seed", range(12))
def test_select_threshold_and_candidates_match_brute_force(seed):
    """Exact-rank forms (no quick bound: pool wanted), lists with counts or holes, extra and spill with planted entries beyond the counts."""
    rng = np.random.default_rng(100 + seed)
    nq, nlists, list_len, l_stride = 3, 5, 4, 6
    k = int(rng.integers(1, 9))
    with_counts = seed % 2 == 0
    lists = np.zeros((nq, nlists * l_stride), np.uint64)
    for q in range(nq):
        lists[q] = random_entries(rng, nlists * l_stride, holes=0.0 if with_counts else 0.3)
    counts = rng.integers(0, list_len + 1, (nq, nlists)).astype(np.uint32) if with_counts else None
    extra = np.stack([random_entries(rng, 3) for _ in range(nq)])
    spill = np.stack([R.pack(np.full(4, 100.0, np.float32), 10_000 + np.arange(4)) for _ in range(nq)])
    spill_count = np.zeros(nq * 16, np.uint32)
    spill_count[::16] = [0, 2, 9]
    delta = np.array([0.0, 0.25, -1.0], np.float32)
    floor_in = np.array([-7.0, -7.0, -7.0], np.float32) if seed % 3 == 0 else None
    take = seed % 4 == 1
    c = R.SelectCase(nq=nq, k=k, q_stride=nlists * l_stride, l_stride=l_stride, nlists=nlists, list_len=list_len, lists=lists.ravel(),
                     list_counts=counts, extra_len=3, extra=extra, spill=spill, spill_cap=4, spill_count=spill_count, delta=delta,
                     tau_floor_in=floor_in, heur_rank=(seed % 3), take_topk=int(take), want_pool=True, want_counts=True)
    st, infos = R.select_reference(c)
    for q in range(nq):
        ent = []
        for l in range(nlists):
            n = list_len if counts is None else int(counts[q, l])
            ent += [int(x) for x in lists[q, l * l_stride:l * l_stride + n]]
        ent += [int(x) for x in extra[q]] + [int(x) for x in spill[q, :min(int(spill_count[16 * q]), 4)]]
        ranked = brute_best_first(ent)
        assert infos[q]["entries"] == len(ranked)
        if delta[q] < 0:
            want = np.float32(np.inf)
        elif len(ranked) >= k:
            a = R.score_of(ranked[k - 1])
            want = np.float32(-np.inf) if a != a else np.float32(np.float32(a) - np.float32(2.0) * delta[q])
            if want != want:
                want = np.float32(-np.inf)
        else:
            want = np.float32(-7.0) if floor_in is not None else np.float32(-np.inf)
        assert np.float32(st["tau_floor_out"][q]).view(np.uint32) == want.view(np.uint32)
        assert st["overflow"][q] == (1 if delta[q] < 0 else 0)
        tau = want
        h = seed % 3
        if delta[q] >= 0 and h and h <= len(ranked) and h <= k:
            th = R.score_of(ranked[h - 1])
            if th == th and th > tau:
                tau = th
        assert np.float32(st["tau_out"][q]).view(np.uint32) == np.float32(tau).view(np.uint32)
        cands = ranked[:k] if take else [e for e in ranked if R.score_of(e) >= want]
        assert st["cands"][q] == cands and st["cand_counts"][q] == len(cands)
        assert st["spill_count"][16 * q] == 0


def test_quick_bound_partition_and_safety():
    """The quick bound ranks the maxima of 64 groups; it never exceeds the exact rank's threshold, equals it when the k best sit in k
    different groups, and gives way to the exact rank when fewer than k groups are non-empty."""
    rng = np.random.default_rng(7)
    nlists, list_len, k = 64, 16, 10
    scores = rng.standard_normal((1, nlists * list_len)).astype(np.float32)
    lists = R.pack(scores, np.arange(nlists * list_len)[None, :])
    slab = np.zeros((4, 8), np.uint16)
    mk = lambda ls: R.SelectCase(nq=1, k=k, q_stride=nlists * list_len, l_stride=list_len, nlists=nlists, list_len=list_len, lists=ls.ravel(),
                                 delta=np.array([0.5], np.float32), slab=slab, queries=np.zeros((1, 8), np.float32), dim=8, nrows=4, k_out=1,
                                 out_stride=1)
    state = dict(tau_out=[None], tau_floor_out=[None], overflow=[0], cand_counts=[None], pool_flag=None, spill_count=[0] * 16, cands={}, answers={},
                 cand_approx={}, cand_exact={}, open={})
    info = R.select_launch(mk(lists), 0, state, False)
    assert info["quick"] and info["nonempty_groups"] == 64
    assert info["proven"] <= info["true_bound"]
    groups = {}
    for i in range(nlists * list_len):
        groups.setdefault(R.quick_group(i), []).append(i)
    assert sorted(len(v) for v in groups.values()) == [16] * 64          # an even partition of the 1,024 slots
    maxima = sorted((float(scores[0, v].max()) for v in groups.values()), reverse=True)
    assert info["proven"] == np.float32(np.float32(maxima[k - 1]) - np.float32(1.0))
    # every entry in ONE group: fewer than k non-empty groups, the exact rank answers
    one = lists.copy()
    keep = np.zeros(nlists * list_len, bool)
    keep[groups[5]] = True
    one[0, ~keep] = np.uint64(R.KEMPTY)
    state["open"] = {}
    info = R.select_launch(mk(one), 0, state, False)
    assert not info["quick"] and info["nonempty_groups"] == 1 and info["proven"] == info["true_bound"]


@pytest.mark.parametrize("seed", range(6))
def test_groups_picks_and_rank_form(seed):
    rng = np.random.default_rng(300 + seed)
    n = [1, 96, 1023, 1024, 700, 130][seed]
    e = R.pack(rng.standard_normal(n).astype(np.float32), 32 * rng.permutation(4 * n)[:n])
    for k in (1, 64, 65, 128):
        picks = R.groups_picks(e, k, True)
        ranked = brute_best_first(e)
        tau, ov, info = R.select_groups_reference(k, e, 0.0, True)
        if info["complete"]:
            assert picks == ranked[:len(picks)]
            assert tau == (R.score_of(ranked[k - 1]) if len(ranked) >= k else np.float32(-np.inf))
        if len(picks) >= k:      # safety, whatever the waves held
            assert tau <= R.score_of(ranked[k - 1])
    # the best 40 groups inside one wave's 128 entries: the rank form at k <= 64 keeps 16 of a wave, so the picks are incomplete
    if n == 1024:
        s = -np.abs(rng.standard_normal(n)).astype(np.float32)
        idx = np.r_[64:84, 576:596]
        assert {R.groups_wave(int(i)) for i in idx} == {1}
        s[idx] = 5.0 + np.arange(40, dtype=np.float32)
        e = R.pack(s, 32 * np.arange(n))
        tau, _, info = R.select_groups_reference(30, e, 0.0, True)
        assert not info["complete"] and tau < brute_score(e, 30)
        assert R.select_groups_reference(10, e, -1.0, True)[:2] == (np.float32(np.inf), 1)
        assert R.select_groups_reference(10, e, 0.0, True, valid=False)[:2] == (np.float32(np.inf), 1)


def brute_score(e, k):
    return R.score_of(brute_best_first(e)[k - 1])


def test_list_cut_and_merge_match_brute_force():
    rng = np.random.default_rng(5)
    lists = np.stack([random_entries(rng, 4, holes=0.4) for _ in range(40)])
    last = brute_best_first(lists[:, -1])
    want = R.score_of(last[0]) if last else np.float32(-np.inf)
    want = np.float32(-np.inf) if want != want else want
    assert R.list_cut_reference(lists).view(np.uint32) == want.view(np.uint32)
    assert R.list_cut_reference(np.full((3, 2), R.KEMPTY, np.uint64)) == np.float32(-np.inf)
    assert R.list_cut_reference(np.zeros((0, 2), np.uint64)) == np.float32(-np.inf)
    for nshards, cc, k in ((1, 1, 1), (2, 30, 30), (8, 90, 1), (8, 128, 128)):
        n = nshards * cc
        rows = rng.permutation(10 * n)[:n].astype(np.uint64)
        approx = R.pack(rng.integers(-3, 4, n).astype(np.float32), rows).reshape(nshards, cc)     # many pass-1 ties: the row decides
        exact = R.pack(rng.standard_normal(n).astype(np.float32), rows).reshape(nshards, cc)
        hole = rng.random((nshards, cc)) < 0.2
        approx[hole] = np.uint64(R.KEMPTY)
        pairs = [(int(a), int(x)) for a, x in zip(approx.ravel(), exact.ravel()) if int(a) != R.KEMPTY]
        pairs.sort(key=functools.cmp_to_key(lambda p, r: before(p[0], r[0])))
        want = brute_best_first(x for _, x in pairs[:cc])[:k]
        assert R.two_pass_merge_reference(approx, exact, cc, k) == want


# ---- the launchers' predicates ----------------------------------------------------------------------------------------------------------

def select_call(k=10, k_out=10, dim=16, slab_f32=0, row_stride=0, finish=True, **kw):
    nq, nlists, list_len = 3, 2, 4
    a = dict(kernel=R.SELECT, nq=nq, k=k, q_stride=nlists * list_len, l_stride=list_len, nlists=nlists, list_len=list_len,
             lists=np.zeros(nq * nlists * list_len, np.uint64), delta=np.zeros(nq, np.float32), tau_out=np.zeros(nq, np.float32),
             overflow=np.zeros(nq, np.uint32))
    if finish:
        a.update(slab=np.zeros((8, max(dim, 8) * 2), np.uint16), queries=np.zeros((nq, max(dim, 8)), np.float32), dim=dim, nrows=8, k_out=k_out,
                 out_stride=64, slab_f32=slab_f32, row_stride=row_stride, out_rows=np.zeros(nq * 64, np.uint32))
    a.update(kw)
    return R.LabCall(**a)


def groups_call(k, nentries, rank_only, dim=16):
    nq = 3
    a = dict(kernel=R.SELECT_GROUPS, nq=nq, k=k, nentries=nentries, rank_only=rank_only, lists=np.zeros(nq * max(nentries, 1), np.uint64),
             delta=np.zeros(nq, np.float32), tau_out=np.zeros(nq, np.float32), anchor_unit=np.ones(nq, np.float32), dim=dim, nrows=8,
             slab=np.zeros((8, 64), np.uint16), queries=np.zeros((nq, 64), np.float32))
    return R.LabCall(**a)


def test_select_predicate():
    for k in (0, 1, 32, 33, 128, 129):
        assert (select_call(k=k, finish=False).check() == R.OK) == R.select_ok(k), k
    assert select_call(k=0).check() == R.INVALID_CONFIG and select_call(k=129).check() == R.INVALID_CONFIG
    for k_out in (0, 1, 64, 65):
        assert (select_call(k_out=k_out).check() == R.OK) == R.select_ok(10, finish=True, k_out=k_out), k_out
    assert select_call(k_out=0).check() == R.INVALID_CONFIG and select_call(k_out=65).check() == R.INVALID_CONFIG
    for dim in (8, 12, 16, 20, 40):
        assert (select_call(dim=dim).check() == R.OK) == R.select_ok(10, finish=True, k_out=10, dim=dim), dim
    assert select_call(dim=12).check() == R.INVALID_CONFIG
    for stride in (0, 64, 128):      # F32 rows: dense only
        assert (select_call(dim=16, slab_f32=1, row_stride=stride).check() == R.OK) == R.select_ok(10, finish=True, k_out=10, dim=16, slab_f32=True, row_stride=stride)
    assert select_call(dim=16, slab_f32=1, row_stride=128).check() == R.INVALID_CONFIG
    assert select_call(dim=16, row_stride=128).check() == R.OK      # (an MRL view of f16 rows)


def test_select_groups_predicate():
    for nentries in (0, 1, 1024, 1025):
        assert (groups_call(10, nentries, 0).check() == R.OK) == R.select_groups_ok(10, nentries, False), nentries
    assert groups_call(10, 0, 0).check() == R.INVALID_CONFIG and groups_call(10, 1025, 1).check() == R.INVALID_CONFIG
    for k in (0, 1, 24, 25, 32, 33):
        assert (groups_call(k, 96, 0).check() == R.OK) == R.select_groups_ok(k, 96, False), k
    assert groups_call(33, 96, 0).check() == R.INVALID_CONFIG
    for k in (1, 64, 65, 128, 129):
        assert (groups_call(k, 96, 1).check() == R.OK) == R.select_groups_ok(k, 96, True), k
    assert groups_call(129, 96, 1).check() == R.INVALID_CONFIG
    assert groups_call(10, 96, 0, dim=12).check() == R.INVALID_CONFIG and groups_call(10, 96, 1, dim=12).check() == R.OK


def test_list_cut_and_merge_predicates():
    cut = lambda nlists, list_len: R.LabCall(kernel=R.LIST_CUT, nlists=nlists, list_len=list_len, lists=np.zeros(max(nlists * list_len, 1), np.uint64),
                                             tau_out=np.zeros(1, np.float32)).check()
    for nlists, list_len in ((0, 1), (5, 0), (5, 32)):
        assert (cut(nlists, list_len) == R.OK) == R.list_cut_ok(nlists, list_len)
    assert cut(5, 0) == R.INVALID_CONFIG

    def merge(nshards, cc, k):
        nq = 3
        n = max(nshards * cc * nq, 1)
        return R.LabCall(kernel=R.TWO_PASS_MERGE, nq=nq, nshards=nshards, cc=cc, k=k, shard_pitch=nq * cc, out_stride=max(k, 1),
                         lists=np.zeros(n, np.uint64), exact_lists=np.zeros(n, np.uint64), out_rows=np.zeros(nq * max(k, 1), np.uint32)).check()
    for nshards, cc, k in ((1, 1, 1), (8, 128, 128), (25, 41, 10), (5, 205, 10), (2, 30, 31), (2, 0, 0)):
        assert (merge(nshards, cc, k) == R.OK) == R.two_pass_merge_ok(nshards, cc, k), (nshards, cc, k)
    assert merge(25, 41, 10) == R.INVALID_CONFIG and merge(5, 205, 10) == R.INVALID_CONFIG      # nshards x cc = 1,025
    assert merge(2, 30, 31) == R.INVALID_CONFIG                                                  # k > cc


def test_lab_argument_checks():
    """What the entry itself refuses before a device is looked for."""
    assert select_call(nq=0).check() == R.INVALID_CONFIG
    assert select_call(valid_queries=4).check() == R.INVALID_CONFIG
    assert select_call(q_stride=7).check() == R.INVALID_CONFIG                  # does not hold 2 lists of 4
    assert select_call(out_stride=5).check() == R.INVALID_CONFIG                # below k_out
    assert select_call(big_pool=1).check() == R.NULL_ARGUMENT                   # no pool_flag
    assert select_call(reset_spill=1).check() == R.NULL_ARGUMENT                # no spill_count
    assert select_call(finish=False, big_pool=0, anchor_unit=np.ones(3, np.float32)).check() == R.INVALID_CONFIG
    assert R.LabCall(kernel=9).check() == R.INVALID_CONFIG

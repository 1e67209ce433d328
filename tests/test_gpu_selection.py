"""ONE launch of a selection kernel at a time, through fsgpu_lab_select (the product's launchers on host arrays), against the plain
reference of tests/selection_ref.py: thresholds bit for bit (the exact anchor within its stated rounding), candidates as sets, answers
and counters exactly.  Every case first asserts FROM THE REFERENCE that its input is in the regime it names, and every launch runs with the
spill counters reset in place, as the product launches it.  Separately from the equality with the restated partitions, every proven
threshold is held to the safety property: it never exceeds (true rank-k score) - 2 delta."""
import functools

import numpy as np
import pytest

import selection_ref as R

pytestmark = pytest.mark.gpu
F32 = np.float32
NROWS = 3000
ROW_BASE = 1000
BIG = F32(1e30)          # planted where nothing may be read: beyond a list's count, beyond the spill count


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    from oracle import oracle
    build()
    oracle.build()


def last_error():
    from frankensearch_amd import _lib
    return _lib.last_error()


@functools.lru_cache(maxsize=None)
def base():
    """(f16 rows [NROWS, 1040] as bits, f32 rows [NROWS, 384], queries [70, 1040]) — made once, never changed."""
    rng = np.random.default_rng(11)
    rows = (rng.standard_normal((NROWS, 1040)) / 8).astype(np.float16)
    rows32 = (rng.standard_normal((NROWS, 384)) / 8).astype(F32)
    q = rng.standard_normal((70, 1040)).astype(F32)
    return rows.view(np.uint16), rows32, q


def bits(x):
    return np.asarray(x, F32).view(np.uint32)


# ---- building a case --------------------------------------------------------------------------------------------------------------------

def distinct_group_positions(rng, pos, n):
    """n of the slot indexes `pos` that feed n different diagonal groups."""
    seen, out = set(), []
    for i in rng.permutation(pos):
        g = R.quick_group(int(i))
        if g not in seen:
            seen.add(g)
            out.append(int(i))
            if len(out) == n:
                return out
    raise AssertionError("not enough groups")


def make_case(seed, nq, k, nlists, list_len, *, l_stride=None, counts=None, holes=0.0, extra_len=0, spill_cap=0, spill_counts=None,
              place="spread", ncand=None, nbest=None, delta=1.0, scores="plain", entries=None, **kw):
    """Lists, extra and spill of nq queries.  The nbest (default k) best entries score around 10 and sit where `place` says; with ncand,
    exactly ncand - nbest more score inside [10 - 2 delta, 10) and everything else below; without, the rest is random.  counts: None (holes
    mark the empty slots), or 'mixed' (0, partial and full lists, entries with enormous scores planted beyond the counts).  entries: cap on
    the number of entries per query (the other slots are holes / beyond the counts)."""
    rng = np.random.default_rng(seed)
    l_stride = l_stride or list_len
    q_stride = nlists * l_stride + 3
    lists32 = nlists * list_len
    nbest = k if nbest is None else nbest
    lists = np.full((nq, q_stride), np.uint64(R.KEMPTY))
    cnt = np.zeros((nq, nlists), np.uint32) if counts else None
    extra = np.full((nq, max(extra_len, 1)), np.uint64(R.KEMPTY))
    spill = np.full((nq, max(spill_cap, 1)), np.uint64(R.KEMPTY))
    sc = np.zeros(nq * R.SPILL_COUNT_STRIDE, np.uint32)
    sc[:] = 0xABAB0000 + np.arange(sc.size)          # the words between the counters are nobody's
    d = np.broadcast_to(np.asarray(delta, F32), (nq,)).copy()
    total = lists32 + extra_len + spill_cap
    for q in range(nq):
        # which slots are entries
        if counts:
            c = rng.integers(0, list_len + 1, nlists)
            c[rng.random(nlists) < 0.3] = list_len
            c[rng.random(nlists) < 0.2] = 0
            if place in ("one_list", "per_list", "one_thread", "one_wave", "one_group"):
                c[:] = list_len
            cnt[q] = c
            live = (np.arange(list_len)[None, :] < c[:, None]).ravel()
        else:
            live = rng.random(lists32) >= holes
        ns = spill_cap if spill_counts is None else int(spill_counts[q])
        sc[q * R.SPILL_COUNT_STRIDE] = ns
        live = np.r_[live, np.ones(extra_len, bool), np.arange(spill_cap) < ns]
        pos = np.flatnonzero(live)
        if entries is not None and len(pos) > entries:
            drop = rng.permutation(pos)[entries:]
            drop = drop[drop < lists32] if not counts else drop[:0]
            live[drop] = False
            pos = np.flatnonzero(live)
        n = len(pos)
        s = np.full(total, BIG, F32)
        nb = min(nbest, n)
        if nb == 0:
            top = []
        elif place == "spread":
            top = distinct_group_positions(rng, pos, nb) if nb <= 64 and len({R.quick_group(int(i)) for i in pos}) >= nb else list(rng.permutation(pos)[:nb])
        else:
            pick = {"one_list": lambda i: i < list_len, "per_list": lambda i: i < lists32 and i % list_len == 0,
                    "one_thread": lambda i: i % 1024 == 77, "one_wave": lambda i: (i % 1024) >> 6 == 3,
                    "one_group": lambda i: R.quick_group(i) == 9}[place]
            cand = [int(i) for i in pos if pick(int(i))]
            assert len(cand) >= nb, (place, len(cand), nb)
            top = cand[:nb]
        rest = np.array(sorted(set(int(i) for i in pos) - set(top)), np.int64)
        rng.shuffle(rest)
        dq = float(max(d[q], 0))
        if scores == "equal":
            s[pos] = F32(2.5)
        else:
            s[top] = F32(10) + (rng.integers(0, 3, len(top)) if scores == "ties" else np.arange(len(top))[::-1]) / F32(64)
            if ncand is not None:
                m = max(min(ncand - nb, len(rest)), 0)
                # (the k-th best is exactly 10 when nbest >= k: the margin is [10 - 2 delta, 10))
                s[rest[:m]] = F32(10) - F32(2 * dq) * (rng.integers(0, 33, m) / F32(32))
                s[rest[m:]] = F32(10 - 2 * dq - 1) - np.abs(rng.standard_normal(len(rest) - m)).astype(F32)
            elif scores == "ties":
                s[rest] = rng.integers(-8, 9, len(rest)).astype(F32) / F32(2)
            else:
                s[rest] = rng.standard_normal(len(rest)).astype(F32) * F32(2)
            if scores == "negative":
                s[pos] = s[pos] - F32(100)
        rows = (ROW_BASE - 40 + rng.permutation(max(total, NROWS + 80))[:total]).astype(np.uint64)
        # (the best entries name real rows of every slab the tests use: rows are unique per query, so they are swapped in)
        inside = lambda r: (r >= ROW_BASE) & (r < ROW_BASE + 2000)
        spare = [int(i) for i in np.flatnonzero(inside(rows)) if int(i) not in set(top)]
        for t in top:
            if not inside(rows[t]) and spare:
                j = spare.pop()
                rows[t], rows[j] = rows[j], rows[t]
        e = R.pack(s, rows)
        if not counts:
            e[:lists32][~live[:lists32]] = np.uint64(R.KEMPTY)
        for l in range(nlists):
            lists[q, l * l_stride:l * l_stride + list_len] = e[l * list_len:(l + 1) * list_len]
            lists[q, l * l_stride + list_len:(l + 1) * l_stride] = R.pack(BIG, 7)          # between the lists
        lists[q, nlists * l_stride:] = R.pack(BIG, 8)
        extra[q, :extra_len] = e[lists32:lists32 + extra_len]
        spill[q, :spill_cap] = e[lists32 + extra_len:]
    c = R.SelectCase(nq=nq, k=k, q_stride=q_stride, l_stride=l_stride, nlists=nlists, list_len=list_len, lists=lists.ravel(), list_counts=cnt,
                     extra_len=extra_len, extra=extra if extra_len else None, spill=spill if spill_cap else None, spill_cap=spill_cap,
                     spill_count=sc, delta=d, reset_spill=1)
    c.__dict__.update(kw)
    return c


def as_finish(c, dim=64, k_out=10, out_stride=None, f32=False, hreduce=0, mrl=False, row_base=ROW_BASE, nrows=NROWS):
    rows, rows32, q = base()
    nv = c.valid_queries or c.nq
    if f32:
        c.slab, c.slab_f32 = np.ascontiguousarray(rows32[:nrows, :dim]), 1
    elif mrl:
        c.slab, c.row_stride = np.ascontiguousarray(rows[:nrows, :384]), 768
    else:
        c.slab = np.ascontiguousarray(rows[:nrows, :dim])
    c.queries = np.ascontiguousarray(q[:nv, :dim + 8])
    c.query_stride = dim + 8
    c.dim, c.nrows, c.row_base, c.hreduce, c.k_out = dim, nrows, row_base, hreduce, k_out
    c.out_stride = out_stride or k_out + 3
    return c


# ---- checking a launch ------------------------------------------------------------------------------------------------------------------

def check(c):
    """Runs the case and holds every output to the reference; returns the reference's per-query facts."""
    ref, infos = R.select_reference(c)
    st, out = R.run_select(c)
    assert st == R.OK, last_error()
    assert np.array_equal(out["spill_count"], np.array(ref["spill_count"], np.uint32)), "spill counters"
    for q in range(c.nq):
        info, opened = infos[q], ref["open"].get(q, set())
        what = f"query {q}: {({a: b for a, b in info.items() if a not in ('first',)})}"
        assert out["overflow"][q] == ref["overflow"][q], what
        if c.pool_flag is not None:
            assert out["pool_flag"][q] == ref["pool_flag"][q], what
        floor = ref["tau_floor_out"][q]
        if c.want_floor:
            if floor is None:
                assert "floor" in opened or bits(out["tau_floor_out"][q]) == R.UNWRITTEN32, what
            else:
                assert bits(out["tau_floor_out"][q]) == bits(floor), (what, out["tau_floor_out"][q])
            # safety, unconditionally: the proven threshold never exceeds (true rank-k score) - 2 delta
            if info.get("true_bound") is not None and bits(out["tau_floor_out"][q]) != R.UNWRITTEN32:
                assert out["tau_floor_out"][q] <= info["true_bound"], what
        if c.want_tau:
            got, want = out["tau_out"][q], ref["tau_out"][q]
            if want is None:
                assert "tau" in opened or bits(got) == R.UNWRITTEN32, what
            elif info.get("anchor"):
                te, tol = info["anchor"]
                p = float(info["proven"])
                assert got >= info["proven"], what
                if te > p + tol:
                    assert abs(float(got) - te) <= tol, (what, got)
                elif te < p - tol:
                    assert bits(got) == bits(info["proven"]), (what, got)
                else:
                    assert bits(got) == bits(info["proven"]) or abs(float(got) - te) <= tol, (what, got)
            else:
                assert bits(got) == bits(want), (what, got)
            if info.get("true_bound") is not None and info.get("gate") is None and not info.get("anchor") and want is not None:
                assert got <= info["true_bound"], what
        untouched = c.big_pool == 2 and info["skipped"]        # a second-chance launch alone leaves an unflagged query as it was
        undefined = "cands" in opened                             # (more live entries than the sorted form holds)
        if c.want_counts and not undefined:
            assert out["cand_counts"][q] == (R.UNWRITTEN32 if untouched else ref["cand_counts"][q]), what
        if c.want_pool and not undefined:
            pool = [int(x) for x in out["pool_out"][q * R.POOL:(q + 1) * R.POOL]]
            if untouched:
                assert all(x == R.UNWRITTEN for x in pool), what
            else:
                cands = ref["cands"][q]
                if len(cands) <= R.POOL:
                    assert sorted(pool) == sorted(cands + [R.KEMPTY] * (R.POOL - len(cands))), what
                else:     # 1,024 of them
                    assert len(set(pool)) == R.POOL and set(pool) <= set(cands), what
        if c.finish:
            os_ = c.out_stride
            packed = [int(x) for x in out["out_packed"][q * os_:(q + 1) * os_]]
            if untouched:
                assert all(x == R.UNWRITTEN for x in packed) and out["out_counts"][q] == R.UNWRITTEN32, what
                continue
            if "answers" in opened or undefined:
                continue
            ans = ref["answers"][q]
            assert packed == ans + [R.KEMPTY] * (os_ - len(ans)), what
            assert out["out_counts"][q] == len(ans), what
            assert [int(x) for x in out["out_rows"][q * os_:(q + 1) * os_]] == [x & 0xFFFFFFFF for x in packed], what
            assert [int(x) for x in bits(out["out_scores"][q * os_:(q + 1) * os_])] == [x >> 32 for x in packed], what
            if c.want_cand_pairs and c.take_topk:
                cs = c.cand_out_stride
                assert [int(x) for x in out["cand_approx_out"][q * cs:q * cs + c.k]] == ref["cand_approx"][q], what
                assert [int(x) for x in out["cand_exact_out"][q * cs:q * cs + c.k]] == ref["cand_exact"][q], what
                assert all(a == R.KEMPTY or e == R.KEMPTY or (a & 0xFFFFFFFF) == (e & 0xFFFFFFFF)
                           for a, e in zip(ref["cand_approx"][q], ref["cand_exact"][q]))
    return infos


SHAPES = {  # name: (nlists, list_len, l_stride, counts, holes)
    "dense": (1, 2048, None, None, 0.0),
    "7x32": (7, 32, None, "mixed", 0.0),
    "512x8": (512, 8, None, "mixed", 0.0),
    "513x5": (513, 5, None, "mixed", 0.0),
    "600x3-holes": (600, 3, 4, None, 0.4),
    "300x4-holes": (300, 4, None, None, 0.5),
    "700x1": (700, 1, 2, "mixed", 0.0),
}
KS = (1, 10, 16, 17, 32, 33, 64, 65, 90, 128)


# ---- select_kernel: the threshold step --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("form", ["gate_floor", "pool", "take_topk"])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_threshold_forms(shape, form):
    """The three forms a sample's selection takes, at every rank class: the heuristic gate with the proven floor (the quick bound where
    it applies), the exact rank with the pool kept, and take_topk."""
    nlists, list_len, l_stride, counts, holes = SHAPES[shape]
    seen = set()
    for n, k in enumerate(KS):
        kw = dict(want_floor=True)
        if form == "gate_floor":
            kw.update(heur_rank=min(k, 5 + k // 8))
        elif form == "pool":
            kw.update(want_pool=True, want_counts=True, tau_floor_in=np.full(4, -3.0, F32))
        else:
            kw.update(take_topk=1, want_pool=True, want_counts=True)
        c = make_case(1000 * n + len(shape), 4, k, nlists, list_len, l_stride=l_stride, counts=counts, holes=holes, extra_len=5, spill_cap=16,
                      spill_counts=[0, 7, 16, 40], delta=[0.25, 0.0, 0.5, -1.0], scores="ties" if n % 2 else "plain", **kw)
        infos = check(c)
        assert all(i["sorted"] == (k > 32) for i in infos)
        seen |= {(i["quick"], i["entries"] >= k) for i in infos}
    if form == "gate_floor":
        assert (True, True) in seen, "no query took the quick bound"
    else:
        assert not any(quick for quick, _ in seen)


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("total", [0, "k-1", "k", 8191, 8192, 8193, 3 * 8192 + 5])
def test_entry_counts(total, k):
    """Entry counts around k, around one pass of 8,192 and over several passes, in a dense list and in lists with holes; the extraction
    form (k = 10) takes more passes, the sorted form (k = 40) holds at most 8,192 LIVE entries."""
    n = {"k-1": k - 1, "k": k}.get(total, total)
    for dense in (True, False):
        if dense:
            live = n if (k <= 32 or n <= 8192) else None
            c = make_case(n + k, 3, k, 1, max(n, 1), entries=n, want_pool=True, want_counts=True, want_floor=True, delta=[0.5, 0.0, 1.0],
                          tau_floor_in=np.full(3, 1.5, F32))
            if n == 0:
                c.nlists = 0
        else:
            slots = max(n, 8)
            live = min(n, 8192) if k > 32 else n
            c = make_case(n + k + 1, 3, k, (slots + 7) // 8, 8, entries=live, holes=0.0, want_pool=True, want_counts=True, want_floor=True,
                          delta=[0.5, 0.0, 1.0])
        infos = check(c)
        for i in infos:
            if live is None:
                assert i["regime"] == "sort_overflow" and i["entries"] == n
            else:
                assert i["entries"] == live and (i["total_slots"] > 8192) == (n > 8192)
                assert i.get("regime") != "sort_overflow"


def test_sorted_form_live_limit():
    """8,192 live entries sort; 8,193 set overflow (which 8,192 were kept is not defined, the threshold stays safe)."""
    for live, over in ((8192, False), (8193, True)):
        c = make_case(live, 3, 90, 1100, 8, entries=live, want_floor=True, want_counts=True, delta=0.5)
        infos = check(c)
        assert all(i["entries"] == live and (i.get("regime") == "sort_overflow") == over for i in infos)


@pytest.mark.parametrize("k", [10, 64])
def test_spill_counts(k):
    """Spill counters of 0, below, at and above the capacity (the kernel reads min(count, cap) slots; enormous scores lie beyond), reset in
    place; the words between the counters are left alone."""
    c = make_case(5, 5, k, 40, 4, counts="mixed", spill_cap=64, spill_counts=[0, 13, 64, 65, 5000], want_pool=True, want_counts=True,
                  want_floor=True, delta=0.25)
    infos = check(c)
    assert [i["total_slots"] - 160 for i in infos] == [0, 13, 64, 64, 64]
    # ... and a full spill area decides the threshold: the best entries are all in it
    c = make_case(6, 3, k, 2, 4, spill_cap=128, spill_counts=[128, 128, 128], place="spread", want_pool=True, want_floor=True, delta=0.25)
    check(c)


@pytest.mark.parametrize("finish", [False, True])
@pytest.mark.parametrize("place", ["one_list", "one_thread", "one_wave", "one_group", "per_list", "spread"])
def test_where_the_best_sit(place, finish):
    """All of the best in one list, one thread's eight slots, one wave's share, one diagonal group (the quick bound must give way to the
    exact rank or stay below it), one per list, spread.  Both the gate form and the finish take the quick bound; the pool form does not."""
    k = 8 if place == "one_thread" else 10
    nlists, list_len = (64, 16) if place != "one_thread" else (1024, 8)
    for form in ("quick", "exact"):
        kw = dict(want_floor=True)
        if not finish:
            kw.update(dict(heur_rank=6) if form == "quick" else dict(want_pool=True, want_counts=True))
        c = make_case(sum(map(ord, place)), 3, k, nlists, list_len, place=place, counts="mixed" if place != "spread" else None,
                      holes=0.3 if place == "spread" else 0.0, delta=0.25, **kw)
        if finish:
            as_finish(c, dim=64, k_out=k)
            c.want_counts = True
            if form == "exact":
                c.heur_rank = 1       # a finish with a gate rank takes the exact rank
        infos = check(c)
        for i in infos:
            assert i["entries"] >= k
            if form == "exact":
                assert not i["quick"] and i["proven"] == i["true_bound"]
            elif place in ("spread", "per_list"):
                assert i["quick"]
            if place == "spread" and form == "quick":
                assert i["proven"] == i["true_bound"]          # k best in k groups: the bound is the rank
            if place == "one_group" and form == "quick" and i["quick"]:
                assert i["proven"] < i["true_bound"]           # one group holds them all: a bound only


def test_one_group_only_gives_way_to_exact_rank():
    """Every entry in ONE diagonal group: fewer than k non-empty groups, so the quick form hands over to the extraction rounds."""
    k = 10
    c = make_case(3, 3, k, 64, 16, delta=0.5, want_floor=True, heur_rank=6)
    lists = c.lists.reshape(c.nq, c.q_stride)
    for i in range(64 * 16):
        if R.quick_group(i) != 9:
            lists[:, i] = np.uint64(R.KEMPTY)
    infos = check(c)
    assert all(i["nonempty_groups"] == 1 and not i["quick"] and i["entries"] == 16 for i in infos)
    as_finish(c, dim=40, k_out=k)
    c.heur_rank = 0
    infos = check(c)
    assert all(i["nonempty_groups"] == 1 and not i["quick"] for i in infos)


@pytest.mark.parametrize("k", [10, 40])
@pytest.mark.parametrize("scores", ["ties", "equal", "negative", "special"])
def test_scores(scores, k):
    """Long runs of equal scores, all equal, negative only; NaN, +inf, -inf, -0.0 and +0.0 among the best k."""
    if scores != "special":
        c = make_case(k, 4, k, 30, 8, counts="mixed", scores=scores, delta=[0.0, 0.25, 0.25, 1.0], want_pool=True, want_counts=True,
                      want_floor=True, heur_rank=6)
        check(c)
        return
    for nent in (k, k + 3):
        c = make_case(k + nent, 4, k, 1, nent, delta=[0.0, 0.0, 0.5, 0.5], want_pool=True, want_counts=True, want_floor=True, heur_rank=1)
        lists = c.lists.reshape(c.nq, c.q_stride)
        special = [np.inf, -np.inf, -0.0, 0.0, np.nan]
        for q in range(4):
            rows = lists[q, :5] & np.uint64(0xFFFFFFFF)
            lists[q, :5] = R.pack(np.array(special, F32), rows)
            lists[q, 5] = (np.uint64(0xFFC12345) << np.uint64(32)) | (lists[q, 5] & np.uint64(0xFFFFFFFF))     # a negative NaN with a payload
            if q % 2:
                lists[q, 6:nent] = R.pack(np.full(nent - 6, -5.0, F32), lists[q, 6:nent] & np.uint64(0xFFFFFFFF))
        infos = check(c)
        assert infos[0]["proven"] == -np.inf or nent > k


@pytest.mark.parametrize("k", [10, 33])
def test_ranks_floors_deltas_padding(k):
    """heur_rank 1, 6, k and one beyond the entries; the floor handed in used (fewer than k entries) and unused; delta 0, typical,
    negative; padding query slots behind valid_queries."""
    for heur in (1, 6, k, 500):
        c = make_case(heur, 6, k, 20, 8, counts="mixed", delta=[0.25, 0.0, 0.25, -1.0, -1.0, -1.0], heur_rank=heur, want_floor=True,
                      tau_floor_in=np.arange(6, dtype=F32) - 2, valid_queries=3)
        few = c.list_counts[1]
        few[:] = 0
        few[0] = min(k - 1, 8)
        infos = check(c)
        assert infos[1]["entries"] < k and infos[1]["proven"] == F32(-1.0)
        assert infos[0]["entries"] >= k and infos[2]["entries"] >= k
        if heur <= k:
            assert infos[0]["gate"] is not None
        else:
            assert all(i["gate"] is None for i in infos)


# ---- select_kernel: the finish ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("ncand", [0, 1, 64, 65, 256, 257, 1024, 1025])
def test_finish_candidate_counts(ncand, f32):
    """Each finisher by candidate count (<= 64, <= 256, more), the pool filled exactly and one past it, with and without pool_flag."""
    for k, k_out in ((10, 10), (40, 10)) if ncand in (65, 1025) else ((10, 10),):
        for flag in (False, True):
            if ncand <= 1:
                c = make_case(ncand, 4, k, 50, 8, counts="mixed", nbest=ncand, ncand=ncand, delta=1.0, tau_floor_in=np.full(4, 9.5, F32))
                for q in range(4):
                    c.list_counts[q, 1:] = 0
                    c.list_counts[q, 0] = 5
                    c.lists.reshape(4, -1)[q, :5] = R.pack(np.r_[np.full(ncand, 10, F32), np.full(5 - ncand, 1, F32)],
                                                           ROW_BASE + 11 * np.arange(5) + q)
            else:
                c = make_case(ncand, 4, k, 300, 8, counts="mixed", ncand=ncand, delta=1.0, spill_cap=32, spill_counts=[0, 32, 9, 64])
            as_finish(c, dim=384 if ncand in (64, 1024) else 40, k_out=k_out, f32=f32)
            c.want_counts = True
            c.want_floor = True
            if flag:
                c.pool_flag = np.full(4, 7, np.uint32)
            infos = check(c)
            assert all(i["ncand"] == ncand for i in infos), [i["ncand"] for i in infos]
            assert all(i["quick"] == (k <= 32) for i in infos) or ncand <= 1
            if ncand <= 1024 and ncand >= 64:
                assert any(i["real"] >= k_out for i in infos)


@pytest.mark.parametrize("dim,f32,mrl", [(8, False, False), (40, False, False), (64, False, False), (384, False, False), (1024, False, False),
                                         (1032, False, False), (128, False, True), (8, True, False), (40, True, False), (384, True, False)])
def test_finish_rescore(dim, f32, mrl):
    """The re-score at dims with and without leftover chunks, on both sides of the query's LDS limit, on an MRL view (dim 128 of rows 768 bytes
    apart) and on F32 rows; every hreduce; k_out 1, 10, 64 with out_stride > k_out; rows outside [row_base, row_base + nrows) dropped."""
    for hreduce, k_out in ((0, 10), (1, 1), (2, 64)):
        c = make_case(dim + hreduce, 3, 10, 60, 8, counts="mixed", ncand=150, delta=0.5)
        as_finish(c, dim=dim, k_out=k_out, f32=f32, mrl=mrl, hreduce=hreduce, nrows=NROWS - 700)
        infos = check(c)
        assert all(i["ncand"] == 150 and 10 <= i["real"] < 150 for i in infos), [i["real"] for i in infos]


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("k", [10, 32, 33, 90])
def test_finish_exact_anchor(k, f32):
    """A sample's selection with the exact anchor (tau_out = max(proven, S unit - delta - |S unit| 1e-6 - 1)), the pool kept, padding slots."""
    c = make_case(k, 6, k, 80, 8, counts="mixed", ncand=3 * k, delta=[1.0, 1.0, 1.0, 0.0, -1.0, -1.0], valid_queries=4, want_pool=True,
                  want_counts=True, want_floor=True)
    as_finish(c, dim=384, k_out=min(k, 64), f32=f32)
    # units that put the anchor above, below and near the proven threshold
    c.anchor_unit = np.array([40.0, 0.001, 12.0, 40.0, 1.0, 1.0], F32)
    infos = check(c)
    assert all(i["anchor"] is not None for i in infos[:4]) and all(i["anchor"] is None for i in infos[4:])
    assert any(i["anchor"][0] > float(i["proven"]) for i in infos[:4]) and any(i["anchor"][0] < float(i["proven"]) for i in infos[:4])


@pytest.mark.parametrize("k", [10, 90, 128])
def test_finish_take_topk_pairs(k):
    """The int8 two-pass finish: the k best entries themselves, re-scored; the candidate pairs of a row-sharded index's shard."""
    c = make_case(k, 4, k, 100, 4, counts="mixed", scores="ties", delta=0.0, take_topk=1, want_counts=True, want_cand_pairs=True,
                  cand_out_stride=k + 2)
    c.list_counts[3, :] = 0
    c.list_counts[3, :3] = 2           # fewer than k entries
    as_finish(c, dim=64, k_out=min(k, 64) if k != 90 else 30)
    infos = check(c)
    assert infos[3]["entries"] == 6 and all(i["entries"] > k for i in infos[:3])


@pytest.mark.parametrize("ncand", [3000, 8192])
def test_finish_big_pool(ncand):
    """More candidates than the pool: the first launch flags the query, the second chance re-scores up to 8,192 of them; unflagged queries
    keep what the first launch wrote.  Then the second-chance launch alone: a skipped query's outputs and spill counter stay untouched."""
    k = 10
    # (1,023 lists of 8 and 8 spilled entries: 8,192 live entries, all that the sorted form holds)
    parts = [make_case(ncand + q, 1, k, 1023, 8, ncand=n, delta=1.0, spill_cap=16, spill_counts=[8]) for q, n in enumerate((ncand, 200, ncand, 64))]
    c = parts[0]
    c.nq = 4
    c.lists = np.concatenate([p.lists for p in parts])
    c.spill = np.concatenate([p.spill for p in parts])
    c.delta = np.concatenate([p.delta for p in parts])
    c.spill_count = np.concatenate([p.spill_count for p in parts])
    c.reset_spill = 0          # (the product's main-pass finish resets nothing: both launches read the same spill area)
    as_finish(c, dim=64, k_out=k)
    c.want_counts = True
    c.big_pool, c.pool_flag = 1, np.full(4, 9, np.uint32)
    infos = check(c)
    assert [i["ncand"] for i in infos if not i["skipped"]] == [ncand, ncand] and [i["skipped"] for i in infos] == [False, True, False, True]
    assert [i["first"]["ncand"] for i in infos] == [ncand, 200, ncand, 64]
    c.big_pool, c.pool_flag, c.reset_spill = 2, np.array([0, 1, 1, 0], np.uint32), 1
    infos = check(c)
    assert [i["skipped"] for i in infos] == [True, False, False, True]


# ---- select_groups_kernel ---------------------------------------------------------------------------------------------------------------

def groups_case(seed, nq, nentries, concentrated=False, nrows=NROWS):
    """Group entries whose rows do not overlap (first rows 32 a + 4 b).  The 200 best of a query begin inside the slab, the others mostly
    past its end; query 1's best group begins at the last multiple of 32 below nrows (nrows mod 32 in 1..16: its second half lies outside)."""
    rng = np.random.default_rng(seed)
    assert 1 <= nrows % 32 <= 16
    cross = 32 * (nrows // 32)
    starts = np.array([32 * a + 4 * b for a in range(300) for b in range(4) if 32 * a != cross])
    inside, outside = starts[starts < nrows], starts[starts >= nrows]
    e = np.zeros((nq, nentries), np.uint64)
    for q in range(nq):
        s = rng.standard_normal(nentries).astype(F32)
        if concentrated and nentries >= 128:
            idx = np.r_[64:64 + 20, 576:576 + 20]
            s[idx] = 5 + np.arange(len(idx), dtype=F32) / 4
        order = np.argsort(-s, kind="stable")
        pool = np.r_[rng.permutation(inside)[:200], rng.permutation(np.r_[outside, inside])]
        _, first = np.unique(pool, return_index=True)
        pool = pool[np.sort(first)]
        g = np.zeros(nentries, np.int64)
        g[order] = pool[:nentries]
        if q == 1:
            g[order[0]] = cross
        e[q] = R.pack(s, ROW_BASE + g)
        e[q, rng.random(nentries) < 0.05] = np.uint64(R.KEMPTY)
    return e


def run_groups(e, k, rank_only, delta, unit=None, f32=False, dim=64, live=None, allow=None, valid=0, hreduce=0, nrows=NROWS - 500):
    nq, nentries = e.shape
    rows, rows32, qs = base()
    nv = valid or nq
    slab = np.ascontiguousarray(rows32[:nrows, :dim] if f32 else rows[:nrows, :dim])
    sc = (0xABAB0000 + np.arange(nq * 16)).astype(np.uint32)
    sc[::16] = 77
    kw = dict(kernel=R.SELECT_GROUPS, nq=nq, k=k, nentries=nentries, rank_only=int(rank_only), lists=e.ravel(), delta=np.asarray(delta, F32),
              tau_out=np.zeros(nq, F32), overflow=np.zeros(nq, np.uint32), spill_count=sc.copy(), reset_spill=1, valid_queries=valid, hreduce=hreduce)
    if not rank_only:
        kw.update(anchor_unit=np.asarray(unit, F32), slab=slab, queries=np.ascontiguousarray(qs[:nv, :dim + 8]), query_stride=dim + 8, dim=dim,
                  nrows=nrows, row_base=ROW_BASE, slab_f32=int(f32))
        words = (nrows + 63) // 64
        for name, m in (("live", live), ("allow", allow)):
            if m is not None:
                kw[name] = np.packbits(np.r_[m, np.zeros(words * 64 - nrows, bool)], bitorder="little").view(np.uint64)
    call = R.LabCall(**kw)
    assert call.run() == R.OK, last_error()
    want_sc = sc.copy()
    want_sc[::16] = 0
    assert np.array_equal(call.spill_count, want_sc)
    infos = []
    for q in range(nq):
        tau, ov, info = R.select_groups_reference(k, e[q], delta[q], rank_only, valid=(valid == 0 or q < valid), unit=None if rank_only else unit[q],
                                                  slab=slab, query=qs[q] if q < nv else None, dim=dim, nrows=nrows, row_base=ROW_BASE,
                                                  hreduce=hreduce, slab_f32=f32, live=live, allow=allow)
        got = call.tau_out[q]
        assert call.overflow[q] == ov, (q, info)
        if info.get("anchor"):
            te, tol = info["anchor"]
            lo = float(R.minus_2delta(R.ranked_score(info["picks"][k - 1]), delta[q])) if len(info["picks"]) >= k else -np.inf
            if te > lo + tol:
                assert abs(float(got) - te) <= tol, (q, got, te)
            elif te < lo - tol:
                assert float(got) == lo, (q, got, lo)
            else:
                assert float(got) == lo or abs(float(got) - te) <= tol
        else:
            assert bits(got) == bits(tau), (q, got, tau)
        # safety of the rank term: never above the true k-th best group maximum - 2 delta
        ranked = R.best_first(e[q])
        if delta[q] >= 0 and (valid == 0 or q < valid) and len(ranked) >= k and not info.get("anchor"):
            assert got <= R.minus_2delta(R.ranked_score(ranked[k - 1]), delta[q])
        infos.append(info)
    return infos


@pytest.mark.parametrize("nentries", [1, 96, 1023, 1024])
def test_select_groups_rank_only(nentries):
    for k in (1, 64, 65, 128):
        for conc in (False, True):
            e = groups_case(nentries + k, 4, nentries, concentrated=conc, nrows=NROWS - 500)
            infos = run_groups(e, k, True, [0.0, 0.5, -1.0, 0.0], valid=3)
            if conc and nentries >= 1023 and k in (64,):
                assert not infos[0]["complete"]          # one wave holds more than its 16: a bound only
            if not conc and nentries >= 1023 and k == 1:
                assert infos[0]["complete"]
            if nentries < k:
                assert len(infos[0]["picks"]) < k


@pytest.mark.parametrize("f32", [False, True])
@pytest.mark.parametrize("nentries", [1, 96, 1023, 1024])
def test_select_groups_anchored(nentries, f32):
    rng = np.random.default_rng(nentries)
    live = rng.random(NROWS - 500) < 0.8
    allow = rng.random(NROWS - 500) < 0.8
    for k in (1, 24, 25, 32):
        for conc in (False, True):
            e = groups_case(nentries + k + 7, 4, nentries, concentrated=conc, nrows=NROWS - 500)
            if nentries >= 96:
                # the best group of query 0 with every row filtered out; of query 1 with its second half past nrows
                g0 = R.row_of(R.best_first(e[0])[0]) - ROW_BASE
                for r in R.group_rows(g0):
                    if r < len(live):
                        live[r] = False
            unit = np.array([30.0, 0.01, 30.0, 30.0], F32)
            infos = run_groups(e, k, False, [0.25, 0.25, -1.0, 0.25], unit=unit, f32=f32, dim=384 if k == 24 else 40, live=live, allow=allow,
                               valid=3, hreduce=k % 3, nrows=NROWS - 500)
            if nentries >= 96:
                assert infos[0]["rows"] >= k and infos[0]["anchor"] is not None
            if nentries == 1:
                assert infos[0]["rows"] <= 8


# ---- list_cut_kernel, two_pass_merge_kernel ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("list_len", [1, 32])
@pytest.mark.parametrize("nlists", [0, 1, 255, 256, 257, 1000])
def test_list_cut(nlists, list_len):
    rng = np.random.default_rng(nlists + list_len)
    for mode in ("mixed", "none_full", "nan_negative"):
        s = rng.standard_normal((nlists, list_len)).astype(F32)
        lists = R.pack(s, rng.permutation(nlists * list_len).reshape(nlists, list_len))
        if mode == "none_full":
            lists[:, -1] = np.uint64(R.KEMPTY)
        elif mode == "mixed":
            lists[rng.random(nlists) < 0.5, -1] = np.uint64(R.KEMPTY)
        else:
            lists[:, -1] = R.pack(np.where(rng.random(nlists) < 0.5, np.nan, -np.abs(s[:, -1]) - 1).astype(F32), np.arange(nlists))
        call = R.LabCall(kernel=R.LIST_CUT, nlists=nlists, list_len=list_len, lists=lists.ravel() if nlists else np.zeros(1, np.uint64),
                         tau_out=np.zeros(1, F32))
        assert call.run() == R.OK, last_error()
        want = R.list_cut_reference(lists)
        assert bits(call.tau_out[0]) == bits(want), (mode, call.tau_out[0], want)
        if mode == "none_full" or nlists == 0:
            assert want == -np.inf


@pytest.mark.parametrize("nshards,cc", [(1, 1), (2, 30), (8, 90), (8, 128)])
def test_two_pass_merge(nshards, cc):
    rng = np.random.default_rng(nshards * cc)
    nq = 5
    pitch = nq * cc + 3
    for k in sorted({1, cc}):
        approx = np.full((nshards, pitch), R.pack(BIG, 1), np.uint64)
        exact = np.full((nshards, pitch), R.pack(BIG, 1), np.uint64)
        for q in range(nq):
            n = nshards * cc
            rows = rng.permutation(20 * n)[:n]
            a = rng.integers(-4, 5, n).astype(F32)                      # pass-1 ties: the row decides
            x = rng.standard_normal(n).astype(F32)
            if q == 1:
                x = -a - np.arange(n, dtype=F32) / F32(4096)            # the exact order reverses the pass-1 order
            ea, ex = R.pack(a, rows), R.pack(x, rows)
            hole = rng.random(n) < (0.3 if q != 2 else 0.97)
            ea[hole] = np.uint64(R.KEMPTY)
            ex[hole] = np.uint64(R.KEMPTY)
            if q == 3:
                ex[rng.random(n) < 0.2] = np.uint64(R.KEMPTY)           # a candidate whose row lay outside its shard's slab
            approx[:, q * cc:(q + 1) * cc] = ea.reshape(nshards, cc)
            exact[:, q * cc:(q + 1) * cc] = ex.reshape(nshards, cc)
        os_ = k + 2
        call = R.LabCall(kernel=R.TWO_PASS_MERGE, nq=nq, nshards=nshards, cc=cc, k=k, shard_pitch=pitch, out_stride=os_, lists=approx.ravel(),
                         exact_lists=exact.ravel(), out_rows=np.zeros(nq * os_, np.uint32), out_scores=np.zeros(nq * os_, F32),
                         out_counts=np.zeros(nq, np.uint32))
        assert call.run() == R.OK, last_error()
        for q in range(nq):
            want = R.two_pass_merge_reference(approx[:, q * cc:(q + 1) * cc], exact[:, q * cc:(q + 1) * cc], cc, k)
            want = want + [R.KEMPTY] * (os_ - len(want))
            assert [int(r) for r in call.out_rows[q * os_:(q + 1) * os_]] == [w & 0xFFFFFFFF for w in want], q
            assert [int(s) for s in bits(call.out_scores[q * os_:(q + 1) * os_])] == [w >> 32 for w in want], q
            assert call.out_counts[q] == sum(w != R.KEMPTY for w in want), q

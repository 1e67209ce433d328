"""tests/lone_scan_ref.py and tests/lone_scan_cases.py without a GPU: the reference's block lists, merged by the reference, are the oracle's
whole-call answers; every case is in the regime it names (a case that is not FAILS); fsgpu_lab_lone_stage_check — which looks at its
arguments before it looks for a device — admits every case of the tables and refuses what the launchers and the kernels cannot take."""
import numpy as np
import pytest

import lone_scan_cases as T
import lone_scan_ref as R

F32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def built():
    R.built()


def by_kind(kind):
    return [c for c in T.scan_cases() if c.kind == kind]


# ---- the order ---------------------------------------------------------------------------------------------------------------------------

def test_sort_keys_are_rank_key():
    rng = np.random.default_rng(5)
    specials = np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, -1.5, -1.5, 2.0, 2.0, 1e-40, -1e-40], F32)
    s = np.where(rng.random(4000) < 0.5, rng.choice(specials, 4000), rng.standard_normal(4000).astype(F32)).astype(F32)
    e = R.pack(s, rng.permutation(16000)[:4000].astype(np.uint64))
    e[rng.random(4000) < 0.1] = np.uint64(R.KEMPTY)
    keys = R.sort_keys(e)
    assert np.all(keys[e == np.uint64(R.KEMPTY)] == 0) and np.all(keys[e != np.uint64(R.KEMPTY)] > 0)
    real = e[e != np.uint64(R.KEMPTY)]
    assert len(set(R.sort_keys(real).tolist())) == real.size
    assert [int(v) for v in real[np.argsort(R.sort_keys(real))[::-1]]] == R.best_first(e)
    nan = R.pack(np.array([np.nan], F32), np.array([9], np.uint64))
    other = np.uint64((0xFFC12345 << 32) | 9)
    assert R.canon_nan(nan)[0] == R.canon_nan(np.array([other]))[0]
    finite = R.pack(np.array([1.5, -np.inf], F32), np.array([3, 4], np.uint64))
    assert np.array_equal(R.canon_nan(np.r_[finite, np.uint64(R.KEMPTY)]), np.r_[finite, np.uint64(R.KEMPTY)])


def test_merge_reference_pads():
    e = R.pack(np.array([1.0, 3.0, 2.0], F32), np.array([5, 6, 7], np.uint64))
    rows, bits, packed, n = R.merge_reference(np.r_[e, np.uint64(R.KEMPTY)], 5, 7)
    assert n == 3 and rows.tolist() == [6, 7, 5] + [0xFFFFFFFF] * 4
    assert bits.tolist() == [int(v) for v in np.array([3.0, 2.0, 1.0], F32).view(np.uint32)] + [0xFFFFFFFF] * 4
    assert packed[3:].tolist() == [R.KEMPTY] * 4


# ---- the reference against the oracle's whole-call answers ---------------------------------------------------------------------------------

def oracle_sample():
    """Random-data cases of the f16 kinds and F32 without an allow bitmap (the oracle's search takes the live bitmap only): every fifth,
    and every one that compacts at the fold-form switch."""
    pool = [c for c in T.scan_cases() if c.data == "random" and c.allow is None and c.kind not in (R.I8, R.I4)]
    return [c for i, c in enumerate(pool) if i % 5 == 0 or (c.regime == "compacts" and c.k in (32, 33, 128, 129))]


@pytest.mark.parametrize("c", oracle_sample(), ids=lambda c: c.name)
def test_reference_lists_merge_to_the_oracle_answer(c):
    from oracle import oracle
    slab, queries = T.arrays_of(c)
    live, _ = T.masks_of(c)
    lists = T.expected_of(c)
    for x in range(c.nq):
        rows, bits, _, n = R.merge_reference(lists[x], c.k, c.k)
        if c.kind == R.F32K:
            orows, oscores = oracle.search_top_k_f32(np.ascontiguousarray(slab[:, :c.dim]), queries[x], c.k, live=live, hreduce=c.hreduce)
        else:
            orows, oscores = oracle.search_top_k(np.ascontiguousarray(slab[:, :c.dim]), queries[x], c.k, live=live, hreduce=c.hreduce)
        assert n == len(orows)
        assert np.array_equal(rows[:n], orows + np.uint32(c.row_base))
        assert np.array_equal(bits[:n], oscores.view(np.uint32))


# ---- every case is in its regime, and the tables hold what they must ----------------------------------------------------------------------

@pytest.mark.parametrize("c", [c for c in T.scan_cases() if c.regime], ids=lambda c: c.name)
def test_scan_case_is_in_its_regime(c):
    live, allow = T.masks_of(c)
    if c.regime == "compacts":
        assert R.gate_walk(c.kind, c.nq, c.tier, c.n, c.grid, c.k, c.row_base, T.scores_of(c), live, allow, enough=1) >= 1
    elif c.regime == "empty blocks":
        assert R.empty_blocks(c.kind, c.nq, c.n, c.grid) >= 1
        lists = T.expected_of(c)
        assert any(np.all(lists[:, b] == np.uint64(R.KEMPTY)) for b in range(c.grid))
    else:
        raise AssertionError(c.regime)


def test_ascending_scores_compact_again_and_again():
    """Ascending by row every row passes the gate: a wave of the 5003-row case compacts many times, in both tiers."""
    for c in T.scan_cases():
        if c.data == "asc" and c.n == T.NMAX and c.kind == R.F16 and c.nq == 1:
            per_wave = c.n // R.WAVES_PER_BLOCK
            assert R.gate_walk(c.kind, c.nq, c.tier, c.n, c.grid, c.k, c.row_base, T.scores_of(c)) >= per_wave // (2 * c.tier) - 1 >= 2
            return
    raise AssertionError("no such case")


@pytest.mark.parametrize("kind", [R.F16, R.F16_HOST_QUERY, R.F16_MQ, R.I8, R.I4, R.F32K], ids=lambda k: R.KIND_NAMES[k])
def test_scan_table_covers_the_edges(kind):
    cases = by_kind(kind)
    assert {c.n for c in cases} >= set(T.NS)
    assert {c.k for c in cases} >= set(T.KS[64]) | set(T.KS[256])
    assert {c.row_base for c in cases} == {0, 1000}
    assert any(c.grid == 1 for c in cases) and any(c.grid == 3 for c in cases)
    assert any(R.WAVES_PER_BLOCK * c.grid > T.tiles_of(c.kind, c.nq, c.n) for c in cases)
    assert {c.data for c in cases} >= {"random", "asc", "desc", "equal", "dup40"} | ({"special"} if kind in T.F16_KINDS + (R.F32K,) else {"extremes"})
    assert {(c.live, c.allow) for c in cases} >= {("flips", None), (None, "flips"), ("flips", "flips"), (None, "none")}
    assert {c.tier for c in cases if c.regime == "compacts"} == {64, 256}
    assert any(c.regime == "empty blocks" for c in cases)


def test_scan_table_covers_the_kinds_own_shapes():
    f16 = by_kind(R.F16)
    assert {c.dim for c in f16 if not c.force_runtime_dim and not c.row_stride} >= {128, 256, 384, 512, 8, 24, 40, 72, 96, 768}
    assert any(c.dim == 384 and c.force_runtime_dim for c in f16) and any(c.dim == 384 and c.plain_loads for c in f16)
    assert any(c.dim == 64 and c.row_stride == 768 for c in f16)
    assert {c.hreduce for c in f16} == {0, 1, 2} and {(c.nq, c.tier) for c in f16} == {(q, t) for q in (1, 2, 4) for t in (64, 256)}
    assert {(c.nq, c.tier, c.dim) for c in by_kind(R.F16_MQ)} == {(q, t, d) for q in (4, 8) for t in (64, 256) for d in (128, 256, 384)}
    assert any(c.n % 16 for c in by_kind(R.F16_MQ))
    for kind in (R.I8, R.I4):
        assert {(c.dim, c.data) for c in by_kind(kind)} >= {(d, s) for d in (128, 256, 384, 512, 768) for s in ("random", "extremes")}
    assert {(c.dim, c.nq) for c in by_kind(R.F32K)} >= {(d, q) for d in (8, 40, 104, 384, 1024) for q in (1, 2, 4)}
    assert {c.dim for c in by_kind(R.F16_HOST_QUERY)} >= {8, 96, 384, 512}


@pytest.mark.parametrize("c", T.merge_cases(), ids=lambda c: c.name)
def test_merge_case_is_in_its_regime(c):
    assert R.merge_regime(c.nlists, c.list_len, c.k, c.lists_sorted) == c.regime
    lists = T.merge_lists(c)
    if c.lists_sorted:
        keys = R.sort_keys(lists)
        assert np.all(keys[:, :, :-1] >= keys[:, :, 1:])          # best first, holes behind
    if c.regime["one_pass"]:
        assert c.resorts is None
        return
    for q in range(c.nq):
        survivors, resorts = R.streaming_plan(lists[q], c.nlists, c.list_len, c.k, c.lists_sorted)
        if c.resorts == 0:
            assert resorts == 0, (survivors, resorts)
        elif c.resorts:
            assert survivors > 4096 and resorts >= c.resorts, (survivors, resorts)


def test_merge_table_covers_the_regimes():
    seen = {tuple(sorted(c.regime.items())) + (("sorted", c.lists_sorted), ("resorts", bool(c.resorts))) for c in T.merge_cases()}
    want = [dict(one_pass=True, per_thread=8, use_heads=False), dict(one_pass=True, per_thread=16), dict(one_pass=True, quick_heads=True),
            dict(one_pass=True, use_heads=True, quick_heads=False), dict(one_pass=False, resorts=False), dict(one_pass=False, resorts=True),
            dict(one_pass=False, use_heads=False, sorted=1), dict(sorted=0, one_pass=True), dict(sorted=0, one_pass=False)]
    for w in want:
        assert any(all(dict(s)[name] == v for name, v in w.items()) for s in seen), w
    adversarial = [c for c in T.merge_cases() if c.content == "adversarial"]
    assert adversarial and all(not c.regime["one_pass"] and c.resorts >= 2 for c in adversarial)
    shapes = {(c.nlists, c.list_len, c.k) for c in T.merge_cases()}
    assert shapes >= {(1, 10, 10), (4, 10, 10), (64, 10, 10), (256, 10, 10), (1024, 8, 8), (1024, 10, 10), (1024, 16, 16), (1025, 16, 16),
                      (2048, 16, 16), (2049, 16, 16), (8, 64, 64), (256, 32, 96), (1, 300, 10), (1, 8192, 256)}
    assert {c.content for c in T.merge_cases()} >= {"random", "tails", "empty", "few", "ties", "adversarial"}
    assert {c.outputs for c in T.merge_cases()} >= {(name,) for name in T.ALL_OUTPUTS}


# ---- the lab entry's verdicts -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", [R.F16, R.F16_HOST_QUERY, R.F16_MQ, R.I8, R.I4, R.F32K], ids=lambda k: R.KIND_NAMES[k])
def test_check_admits_every_scan_case(kind):
    for c in by_kind(kind):
        assert R.scan_ok(c.kind, c.nq, c.tier, c.dim, c.n, c.k, c.grid, c.row_stride, c.force_runtime_dim, c.plain_loads, c.hreduce), c.name
        assert T.lab_call(c).check() == R.OK, c.name


def test_check_admits_every_merge_case():
    for c in T.merge_cases():
        assert R.merge_ok(c.nq, c.nlists, c.list_len, c.k, c.out_stride, c.l_stride, c.q_stride, c.lists_sorted), c.name
        assert T.merge_lab_call(c).check() == R.OK, c.name


def scan_args(**kw):
    d = dict(kind=R.F16, nq=1, tier=64, dim=128, nrows=100, k=10, grid=3, row_stride=0, force_runtime_dim=0, plain_loads=0, hreduce=0)
    d.update(kw)
    return d


SCAN_REFUSALS = [
    ("k above the tier", scan_args(k=65)), ("k above the tier 256", scan_args(tier=256, k=257)), ("k = 0", scan_args(k=0)),
    ("grid 0", scan_args(grid=0)), ("grid above 4096", scan_args(grid=4097)), ("nrows 0", scan_args(nrows=0)),
    ("tier 128", scan_args(tier=128, k=10)), ("three queries", scan_args(nq=3)), ("eight queries, f16", scan_args(nq=8)),
    ("dim 0", scan_args(dim=0)), ("dim 12", scan_args(dim=12)), ("dim 4104", scan_args(dim=4104)),
    ("row_stride below a row", scan_args(row_stride=240)), ("row_stride 264", scan_args(row_stride=264)),
    ("hreduce 3", scan_args(hreduce=3)),
    ("host query, two queries", scan_args(kind=R.F16_HOST_QUERY, nq=2)), ("host query, dim 520", scan_args(kind=R.F16_HOST_QUERY, dim=520)),
    ("host query, runtime dim flag", scan_args(kind=R.F16_HOST_QUERY, force_runtime_dim=1)),
    ("mq, two queries", scan_args(kind=R.F16_MQ, nq=2)), ("mq, dim 512", scan_args(kind=R.F16_MQ, nq=4, dim=512)),
    ("mq, strided", scan_args(kind=R.F16_MQ, nq=4, dim=128, row_stride=512)), ("mq, plain loads", scan_args(kind=R.F16_MQ, nq=4, plain_loads=1)),
    ("i8, dim 64", scan_args(kind=R.I8, dim=64)), ("i8, two queries", scan_args(kind=R.I8, nq=2)), ("i8, strided", scan_args(kind=R.I8, row_stride=256)),
    ("i4, dim 640", scan_args(kind=R.I4, dim=640)), ("i4, tier 32", scan_args(kind=R.I4, tier=32)),
    ("f32, dim 12", scan_args(kind=R.F32K, dim=12)), ("f32, eight queries", scan_args(kind=R.F32K, nq=8)),
    ("f32, row_stride below a row", scan_args(kind=R.F32K, row_stride=256)),
]


@pytest.mark.parametrize("what,a", SCAN_REFUSALS, ids=[w for w, _ in SCAN_REFUSALS])
def test_check_refuses_scans(what, a):
    assert not R.scan_ok(a["kind"], a["nq"], a["tier"], a["dim"], a["nrows"], a["k"], a["grid"], a["row_stride"], a["force_runtime_dim"],
                         a["plain_loads"], a["hreduce"])
    big = np.zeros(1 << 16, np.uint64)
    call = R.LabCall(slab=big, queries=big, partial=big, **a)
    assert call.check() == R.INVALID_CONFIG
    assert call.run() == R.INVALID_CONFIG            # refused before a device is looked for: nothing is launched


def test_check_refuses_short_bitmaps_and_null_pointers():
    big = np.zeros(1 << 16, np.uint64)
    ok = scan_args(nrows=130)
    assert R.LabCall(slab=big, queries=big, partial=big, live=big, bitmap_words=3, **ok).check() == R.OK
    assert R.LabCall(slab=big, queries=big, partial=big, live=big, bitmap_words=2, **ok).check() == R.INVALID_CONFIG
    assert R.LabCall(slab=big, queries=big, partial=big, allow=big, bitmap_words=0, **ok).check() == R.INVALID_CONFIG
    assert R.LabCall(slab=big, queries=big, partial=big, **ok).check() == R.OK
    for missing in ("slab", "queries", "partial"):
        kw = dict(slab=big, queries=big, partial=big)
        del kw[missing]
        assert R.LabCall(**kw, **ok).check() == R.NULL_ARGUMENT
    assert R.LabCall(kind=7).check() == R.INVALID_CONFIG
    assert R.LabCall(kind=R.MERGE, nq=1, nlists=4, list_len=10, k=10, l_stride=10, q_stride=40, out_stride=10).check() == R.NULL_ARGUMENT


def merge_args(**kw):
    d = dict(nq=1, nlists=4, list_len=10, k=10, out_stride=10, l_stride=10, q_stride=40, lists_sorted=1)
    d.update(kw)
    return d


MERGE_REFUSALS = [
    ("out_stride below k", merge_args(out_stride=9)), ("k = 0", merge_args(k=0)), ("k = 257", merge_args(k=257, out_stride=257)),
    ("no lists", merge_args(nlists=0)), ("empty lists", merge_args(list_len=0)), ("no queries", merge_args(nq=0)),
    ("l_stride below list_len", merge_args(l_stride=9)), ("q_stride below the lists", merge_args(q_stride=39)),
    ("lists_sorted 2", merge_args(lists_sorted=2)), ("out_stride above 4096", merge_args(out_stride=4097)),
]


@pytest.mark.parametrize("what,a", MERGE_REFUSALS, ids=[w for w, _ in MERGE_REFUSALS])
def test_check_refuses_merges(what, a):
    assert not R.merge_ok(**a)
    call = R.LabCall(kind=R.MERGE, lists=np.zeros(1 << 12, np.uint64), out_packed=np.zeros(1 << 13, np.uint64), **a)
    assert call.check() == R.INVALID_CONFIG
    assert call.run() == R.INVALID_CONFIG

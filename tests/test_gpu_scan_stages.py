"""ONE launch of a scan stage at a time, through fsgpu_lab_scan_stage (the product's launchers on host arrays), against the plain
reference of tests/scan_stage_ref.py: exactly which (query, row) pairs come out — lists and spill area together, as a multiset — and with
which score (bit for bit on int8 rows; within gamma = dim 2^-23 |q| |r| of the f64 dot on f16 rows, whose thresholds are placed in a gap
of 4 gamma so that the expected SET is exact too).  Every instantiation the launchers' predicates accept is run (test_instantiation);
the edges — slab lengths around a tile, bitmaps, the MRL stride, special rows, spill and overflow, and the launch parameters that must
not change the answer — run on one instantiation per code path (PATHS)."""
import functools
import os

import numpy as np
import pytest

import scan_stage_ref as S

pytestmark = pytest.mark.gpu
RATIOS = {}        # instantiation -> largest |a - s64| / gamma seen in this run
NROWS = 5003       # several rounds at grid 8 for every tile size; no multiple of any
INF = np.float32(np.inf)


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    build()
    print("instantiations:", " ".join(S.inst_id(i) for i in S.instantiations()))
    yield
    path = os.environ.get("FSGPU_SCAN_RATIOS")   # (how profiles/scan_stages/ratios.txt is made)
    if path:
        with open(path, "a") as f:
            for key, ratio in sorted(RATIOS.items()):
                f.write(f"{key:28s} max |a - s64| / bound {ratio:.4f}\n")


# One instantiation per code path: both LDS-query shapes on both element types and all three stages; the register-query kernel's chunk
# loop on f16 rows (32-row tiles), its split loop with 128-row tiles at an even and an odd number of query tiles, the chunk loop on
# neg-tau accumulators (5 tiles of 384 bytes), 32-row tiles on int8 rows, the thresholded samples of each loop and the group maxima.
PATHS = [(S.LDS, 384, 2, 0, 2), (S.LDS, 256, 2, 2, 2), (S.LDS, 128, 1, 0, 2), (S.LDS, 384, 1, 2, 2), (S.LDS, 64, 2, 2, 1), (S.LDS, 384, 1, 0, 1),
         (S.LDS, 256, 1, 2, 0),
         (S.REG, 384, 2, 3, 2), (S.REG, 256, 2, 2, 2), (S.REG, 384, 1, 4, 2), (S.REG, 384, 1, 3, 2), (S.REG, 384, 1, 5, 2), (S.REG, 256, 1, 5, 2),
         (S.REG, 768, 1, 3, 2), (S.REG, 512, 1, 4, 2), (S.REG, 384, 1, 4, 1), (S.REG, 384, 2, 2, 1), (S.REG, 256, 1, 3, 1),
         (S.REG, 384, 1, 4, 3), (S.REG, 256, 1, 5, 3)]
assert set(PATHS) <= set(S.instantiations())


# ---- data: made once per (dim, element type), never changed -----------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def base(dim, eb, levels4=False):
    """(rows [NROWS, 2 dim], queries [1920, dim], needle [dim]) as the kernels read them.  Rows are random directions; every query leans
    towards one common direction, and the needle IS that direction: it scores far above any threshold against every query.  Columns
    dim.. of the rows are what an MRL view must not read."""
    rng = np.random.default_rng(1000 * dim + 10 * eb + int(levels4))
    c = rng.standard_normal(dim)
    c /= np.linalg.norm(c)
    rows = rng.standard_normal((NROWS, 2 * dim))
    rows[:, :dim] /= np.linalg.norm(rows[:, :dim], axis=1, keepdims=True)
    q = 0.6 * c[None, :] + 0.8 * rng.standard_normal((1920, dim)) / np.sqrt(dim)
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    if eb == 2:
        rows[:, dim:] *= 30.0
        return rows.astype(np.float16).view(np.uint16), q.astype(np.float16).view(np.uint16), c.astype(np.float16).view(np.uint16)
    lim = 7 if levels4 else 127
    quant = lambda x: np.clip(np.rint(x / np.abs(x).max(axis=-1, keepdims=True) * lim), -lim, lim).astype(np.int8)
    rows8 = quant(rows[:, :dim])
    return np.concatenate([rows8, np.full_like(rows8, lim)], axis=1), quant(q), quant(c)


def sample_count(nrows, stride):
    """As many sample groups as begin below nrows."""
    return ((nrows + 63) // 64 - 1) // stride + 1


def run_and_check(inst, nrows=NROWS, grid=8, *, groups=1, reverse=0, sbs=0, live=None, allow=None, tau_mode="gap", rank=20, slots=16,
                  spill_cap=256, row_base=0, mrl=False, want_counts=0, stride=3, needles=True, special="", levels4=False, lds_skip=True, what=""):
    """One launch of `inst` on the first nrows rows, and everything the stage contract says about its outputs."""
    kernel, dim, eb, variant, stage = inst
    G = S.group_queries(kernel, variant)
    nq = G * groups
    rows_all, q_all, needle = base(dim, eb, levels4)
    slab = rows_all[:nrows].copy()
    queries = q_all[:nq]
    sampled = (kernel == S.LDS and stage < 2) or (kernel == S.REG and stage != 2)
    # (the LDS-query main pass skips the groups of the stage-1 sample; lds_skip = False: there was none, it visits everything)
    count = sample_count(nrows, stride) if (sampled or (kernel == S.LDS and lds_skip)) else 0
    visited = S.visited_rows(kernel, stage, nrows, stride, count)
    live = np.ones(nrows, bool) if live is None else live[:nrows].copy()
    allow = np.ones(nrows, bool) if allow is None else allow[:nrows].copy()
    use_live, use_allow = not live.all(), not allow.all()
    planted = 0
    if needles:
        # one needle per row-in-128 position, each in another tile where the slab has that many: every lane, register and query tile of
        # the C fragment holds a passing score at least once
        for p in range(128):
            cand_rows = np.flatnonzero(visited & (np.arange(nrows) % 128 == p))
            if len(cand_rows):
                r = cand_rows[(p * 5) % len(cand_rows)]
                slab[r, :dim] = needle
                live[r] = allow[r] = True
                planted += 1
    if special:   # f16: a row with one NaN element (its lane's three other rows must still pass), an all-zero row, a row of f16 max
        for r0 in (4, 64 + 33, 128 + 77):
            if r0 + 3 < nrows:
                slab[r0 + 1, 7] = 0x7E00
                slab[r0 + 2, :dim] = 0
                if special == "max":
                    slab[r0 + 3, :dim] = 0x7BFF
                live[r0:r0 + 4] = allow[r0:r0 + 4] = True
    valid = live & allow
    mask = visited & valid
    if eb == 2:
        s64, gamma = S.scores_f16(slab, queries)
    else:
        s64, gamma = S.scores_int(slab, queries).astype(np.float64), None
    tau = np.full(nq, -INF, np.float32)
    if stage in (1, 2):
        if tau_mode in ("gap", "low"):
            for q in range(nq):
                # (ranks count from below the needles, which all score the same)
                r = planted + (rank if tau_mode == "gap" or q % 3 else 3)          # "low": a third of the queries keep a high threshold
                if eb == 2:
                    gm = np.nanmax(np.where(mask & np.isfinite(s64[q]), gamma[q], 0.0))
                    tau[q] = S.gap_tau(s64[q], mask, r, gm)[0]
                else:
                    kth = np.sort(s64[q][mask])[::-1][r - 1]
                    tau[q] = np.float32(kth + 0.5) if q % 2 else np.float32(kth)      # odd: between two scores; even: the >= edge
        if tau_mode == "gap":
            tau[nq - 16:] = INF          # padding queries of the last group: nothing is appended
            tau[5] = np.nan              # nothing is appended
    kw = dict(grid=grid, slots=slots, spill_cap=spill_cap, groups=groups if groups > 1 else 0, live=S.bitmap_words(live) if use_live else None,
              allow=S.bitmap_words(allow) if use_allow else None, group_stride=stride, group_count=count, row_base=row_base, reverse=reverse,
              side_by_side=sbs, want_counts=want_counts)
    if mrl:
        out = S.run_scan(kernel, variant, stage, eb, dim, slab, queries, tau, row_stride=2 * dim * eb, **kw)
    else:
        out = S.run_scan(kernel, variant, stage, eb, dim, np.ascontiguousarray(slab[:, :dim]), queries, tau, **kw)
    key = S.inst_id(inst)

    def check_scores(q, a, rows):
        if eb == 1:
            assert np.array_equal(a.view(np.uint32), s64[q, rows].astype(np.float32).view(np.uint32)), (key, what, "score bits", q)
        elif len(rows):
            err, g = np.abs(a.astype(np.float64) - s64[q, rows]), gamma[q, rows]
            assert np.all(err[g == 0] == 0), (key, what, "an all-zero row scores exactly 0", q)
            ratio = float(np.max(err[g > 0] / g[g > 0], initial=0.0))
            RATIOS[key] = max(RATIOS.get(key, 0.0), ratio)
            assert ratio <= 1.0, (key, what, "|a - s64| / gamma", ratio, q)

    if stage == 0:
        dense = out["dense"]
        assert not np.any(dense == S.UNWRITTEN), (key, what, "a dense slot was not written")
        _, rows, ok = S.dense_expected(np.zeros((1, nrows), np.float32), valid, nrows, stride, count, row_base)
        assert np.all(dense[:, ~ok] == S.KEMPTY) and not np.any(dense[:, ok] == S.KEMPTY), (key, what, "kEmpty exactly at the invalid rows")
        a, r = S.unpack(dense[:, ok])
        assert np.array_equal(r, np.broadcast_to(row_base + rows[ok], r.shape)), (key, what, "the row the layout names")
        for q in range(nq):
            if eb == 1 or np.all(np.isfinite(s64[q, rows[ok]])):
                check_scores(q, a[q], rows[ok])
        return
    if stage == 3:
        cand = out["cand"]
        assert not np.any(cand == S.UNWRITTEN), (key, what, "a group-maxima slot was not written")
        for grp in range(groups):
            rev = reverse ^ (grp & 1) if groups > 1 and not sbs else reverse
            qs = slice(grp * G, (grp + 1) * G)
            best, have, classes = S.group_maxima_expected(s64[qs].astype(np.int64), valid, nrows, grid, stride, count, rev)
            got = cand[qs]
            assert np.array_equal(got != S.KEMPTY, have), (key, what, "kEmpty exactly where a class has no valid row")
            a, r = S.unpack(got)
            assert np.array_equal(a[have].view(np.uint32), best[have].astype(np.float32).view(np.uint32)), (key, what, "group maxima")
            for b in range(grid):
                for fk in range(4):
                    for q in np.flatnonzero(have[:, b, fk])[:: max(1, G // 16)]:
                        g = int(r[q, b, fk]) - row_base - fk * 4
                        assert g in classes[(b, fk)], (key, what, "the reported group is not in the block's class", q, b, fk, g)
                        lanes = np.array([g + fk * 4 + i for i in range(4)] + [g + 16 + fk * 4 + i for i in range(4)])
                        lanes = lanes[valid[lanes]]
                        assert s64[grp * G + q, lanes].max() == best[q, b, fk], (key, what, "the reported group does not attain the score")
        return
    taken, lens, spills = S.collect(out, nq, grid, slots, spill_cap)
    expect = S.expected_rows(s64, tau, mask)
    # the block every visited row belongs to, by direction
    blocks = {}
    for rev in {reverse, reverse ^ 1} if (groups > 1 and kernel == S.REG and not sbs) else {reverse}:
        blk = np.full(nrows, -1)
        vr = np.flatnonzero(visited)
        blk[vr] = [S.row_block(int(r), kernel, variant, stage, dim, eb, grid, nrows, stride, count, rev) for r in vr]
        blocks[rev] = blk
    both = 0
    for q in range(nq):
        grp = q // G
        rev = reverse ^ (grp & 1) if (groups > 1 and kernel == S.REG and not sbs) else reverse
        in_lists = out["cand"][q][taken[q]]
        got = np.concatenate([in_lists, spills[q]])
        a, rows = S.unpack(got)
        rows = rows - row_base
        assert np.all((rows >= 0) & (rows < nrows)), (key, what, "a row outside the slab", q)
        nspill = int(out["spill_count"][q, 0])
        assert nspill == len(expect[q]) - int(lens[q].sum()), (key, what, "spill_count = passing pairs - list lengths", q, nspill, len(expect[q]), int(lens[q].sum()))
        assert int(out["overflow"][q]) == int(nspill > spill_cap), (key, what, "overflow = spill_count > spill_cap", q)
        order = np.sort(rows)
        if nspill <= spill_cap:
            assert np.array_equal(order, expect[q]), (key, what, "lists + spill != the expected set", q, np.setxor1d(order, expect[q])[:8])
        else:
            both += 1
            assert len(np.unique(rows)) == len(rows) and np.all(np.isin(rows, expect[q])) and len(rows) == int(lens[q].sum()) + spill_cap, \
                (key, what, "an overflowed query still reports a duplicate-free subset", q)
        check_scores(q, a, rows)
        # a list holds rows of its own block's tiles only
        lrow = S.unpack(out["cand"][q][taken[q]])[1] - row_base
        lblk = np.broadcast_to(np.arange(grid)[:, None], taken[q].shape)[taken[q]]
        assert np.array_equal(blocks[rev][lrow], lblk), (key, what, "an entry in another block's list", q)
    return both


# ---- every instantiation ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", S.instantiations(), ids=S.inst_id)
def test_instantiation(inst):
    """5,003 rows at grid 8 (ragged first / last rounds), both bitmaps at 50 %, row_base != 0, 128 planted needles, thresholds at rank 20
    (f16: in a gap of 4 gamma; int8: between two scores and exactly ON a score, alternating), padding queries (tau = +inf), a NaN tau."""
    rng = np.random.default_rng(7)
    live, allow = rng.random(NROWS) < 0.5, rng.random(NROWS) < 0.5
    kernel, dim, eb, variant, stage = inst
    run_and_check(inst, live=live, allow=allow, row_base=1_000_000, want_counts=int(kernel == S.REG and stage != 3 and variant % 2 == 1),
                  reverse=int(kernel == S.REG and variant >= 4), what="base")


# ---- edges, on one instantiation per code path ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("inst", PATHS, ids=S.inst_id)
def test_slab_lengths_around_a_tile(inst):
    """1 row to one row past a whole round (TR x grid +- 1) at grid 3, tau = -inf: every live row must come out through lists + spill."""
    kernel, dim, eb, variant, stage = inst
    tr = S.tile_rows(kernel, variant, stage, dim, eb)
    rng = np.random.default_rng(11)
    live = rng.random(NROWS) < 0.5
    for nrows in sorted({1, 31, 32, 33, 63, 64, 65, 127, 128, 129, tr * 3 - 1, tr * 3 + 1}):
        run_and_check(inst, nrows, 3, live=live, tau_mode="neginf", slots=32, spill_cap=nrows, stride=1 if nrows < 200 else 2, needles=False,
                      reverse=nrows & 1, lds_skip=False, what=f"nrows {nrows}")


def bitmap_patterns(n):
    rng = np.random.default_rng(13)
    half = rng.random(n) < 0.5
    edge = rng.random(n) < 0.5
    edge[0:64] = False            # an all-zero word ...
    edge[64:128] = True           # ... next to an all-ones word
    edge[128:160] = True          # a word whose lower half is set and whose upper half is clear: pair_row0 & 32 picks the half
    edge[160:192] = False
    edge[192:224] = False
    edge[224:256] = True
    return half, edge


@pytest.mark.parametrize("inst", PATHS, ids=S.inst_id)
def test_bitmaps_are_honoured_at_every_position(inst):
    """No bitmap, live only, allow only, both at 50 %; words of all zeros, all ones, one half set; the partial last word (715 rows).
    tau = -inf: every position of every tile reports, so a bit read from the wrong half or the wrong word shows."""
    n = 715
    half, edge = bitmap_patterns(n)
    for live, allow, what in ((None, None, "none"), (half, None, "live"), (None, edge, "allow"), (edge, half, "both"), (half, ~half, "disjoint")):
        run_and_check(inst, n, 3, live=live, allow=allow, tau_mode="neginf", slots=32, spill_cap=n, stride=2, needles=False, lds_skip=False, what=what)


@pytest.mark.parametrize("inst", PATHS, ids=S.inst_id)
def test_launch_parameters_do_not_change_the_answer(inst):
    """reverse, groups 1 / 2 / 3 (each group has its own queries and thresholds: per-group offsets of queries, tau, lists, spill and
    overflow), side by side on grids the groups do not divide, grids 1, 3, 8, 40 and one larger than the number of tiles."""
    kernel, dim, eb, variant, stage = inst
    n = 2100
    reg_main = kernel == S.REG and stage == 2
    for grid, groups, reverse, sbs in ((1, 1, 0, 0), (3, 2, 1, 0), (8, 3, 0, 0), (8, 3, 1, 1), (5, 2, 0, 1), (40, 1, 1, 0), (150, 2, 0, 0)):
        if sbs and not reg_main:
            sbs = 0
        run_and_check(inst, n, grid, groups=groups, reverse=reverse, sbs=sbs, slots=8 if grid < 8 else 4, spill_cap=256, rank=10,
                      want_counts=int(kernel == S.REG and stage != 3 and grid % 2 == 1), what=f"grid {grid} groups {groups} reverse {reverse} sbs {sbs}")


@pytest.mark.parametrize("inst", [i for i in PATHS if i[4] in (1, 2)], ids=S.inst_id)
def test_spill_and_overflow(inst):
    """slots = 2, spill_cap = 8 and thresholds at rank 60 for two queries in three: both branches of the spill path are taken; what
    is present is a duplicate-free subset of the expected set and the counters say exactly what is missing."""
    both = run_and_check(inst, 1500, 3, tau_mode="low", rank=60, slots=2, spill_cap=8, needles=False, what="spill")
    assert both > 0, "no query overflowed its spill area: the test does not reach that branch"


@pytest.mark.parametrize("inst", [i for i in PATHS if i[2] == 2], ids=S.inst_id)
def test_special_f16_rows(inst):
    """A row with a NaN element never passes and does not take the rows of its lane with it; a zero row; a row of f16 max."""
    run_and_check(inst, 715, 3, tau_mode="neginf", slots=32, spill_cap=715, stride=1, needles=False, special="max", lds_skip=False, what="special, tau -inf")
    run_and_check(inst, 1500, 3, special="nan and zero", what="special, rank 20")   # (a row of f16 max has no gap of 4 gamma next to it)


@pytest.mark.parametrize("inst", [i for i in PATHS if i[0] == S.LDS or i[1] in (256, 384)], ids=S.inst_id)
def test_mrl_view_reads_only_the_prefix(inst):
    """row_stride = 2 x the row's bytes: the first dim elements of rows twice as long (the rest would change every score)."""
    run_and_check(inst, 1500, 5, mrl=True, row_base=77, what="mrl")


@pytest.mark.parametrize("inst", [i for i in PATHS if i[2] == 1 and i[1] in (256, 384)], ids=S.inst_id)
def test_4bit_levels(inst):
    """Rows and queries of levels -7..7 (the batched 4-bit pass 1 runs on the int8 kernels): scores bit for bit."""
    run_and_check(inst, 1500, 5, levels4=True, what="4-bit levels")


# ---- the query preparation --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dim", [64, 384])
def test_prepared_queries_stay_within_delta(dim, oracle):
    """The certificate's premise (mfma_scan.hip's header): for every row of a 2,500-row slab, |dense approximate score of the prepared
    f16 query - the exact-order f32 score| <= delta_q.  Queries with f16-subnormal elements, a large norm, zeros, a non-finite element."""
    n = 2500
    rows16 = np.ascontiguousarray(base(dim, 2)[0][:n, :dim])
    rng = np.random.default_rng(17)
    q = rng.standard_normal((40, dim)).astype(np.float32) / np.float32(np.sqrt(dim))
    q[1] *= 300.0                      # a large norm
    q[2, ::3] = 3e-6                   # f16-subnormal elements
    q[3] = 1e-7                        # all of them
    q[4] = 0.0                         # a zero query: skip marker
    q[5, 9] = np.inf                   # non-finite: skip marker
    q[6, 9] = np.nan
    q[7, 0] = 70000.0                  # above f16 max: skip marker
    r64 = rows16.view(np.float16).astype(np.float64)
    max_norm = np.float32(np.sqrt((r64 * r64).sum(axis=1)).max() * 1.0001)
    prepared, delta = S.run_prepare(q, 64, 2, max_norm=max_norm)
    assert np.all(delta[[4, 5, 6, 7]] < 0) and np.all(delta[40:] < 0) and np.all(prepared[40:] == 0), "skip markers and zero padding"
    real = [i for i in range(40) if i not in (4, 5, 6, 7)]
    assert np.all(delta[real] > 0)
    with np.errstate(over="ignore", invalid="ignore"):
        keep = [i for i in range(40) if i != 6]      # (a NaN's payload is not part of the contract)
        assert np.array_equal(prepared[keep], q[keep].astype(np.float16).view(np.uint16)), "the f16 rounding of the queries"
    # the kernel's delta is the header's formula (it may only sit above the f64 value: it inflates |q| by 1.0001)
    want = S.prepare_delta_bound(q[real], float(max_norm))
    assert np.all(delta[real] >= want * (1 - 1e-6)) and np.all(delta[real] <= want * 1.001)
    tau = np.zeros(64, np.float32)
    out = S.run_scan(S.LDS, 0, 0, 2, dim, rows16, prepared, tau, grid=8, group_stride=1, group_count=(n + 63) // 64)
    a, r = S.unpack(out["dense"][:, :n])
    assert np.array_equal(r, np.broadcast_to(np.arange(n), r.shape))
    worst = 0.0
    for i in real:
        exact = oracle.gather_dot(rows16, q[i], np.arange(n, dtype=np.uint32))
        ratio = float(np.max(np.abs(a[i].astype(np.float64) - np.asarray(exact, np.float64))) / delta[i])
        worst = max(worst, ratio)
        assert ratio <= 1.0, ("|a - s| / delta", i, ratio)
    RATIOS[f"prepare-d{dim}-f16 (delta)"] = worst


@pytest.mark.parametrize("dim", [128, 384])
def test_prepared_int8_and_4bit_queries_are_the_oracles(dim, oracle):
    rng = np.random.default_rng(19)
    q = rng.standard_normal((21, dim)).astype(np.float32)
    q[1] *= 1e4
    q[2] = 0.0
    q[3, 4] = np.nan
    q[4] = 1e-12                   # below the 4-bit floor of 1e-9: levels 0 there, scaled on the int8 side
    q[5, :] = np.round(q[5] * 2) / 2 + 0.5     # ties: round half away from zero
    for bits in (8, 4):
        prepared, delta = S.run_prepare(q, 64, 1, bits=bits)
        assert np.all(delta[:21] == 0) and np.all(delta[21:] < 0) and np.all(prepared[21:] == 0)
        for i in range(21):
            want = oracle.quantize_query_i8(q[i]) if bits == 8 else S.levels_4bit(oracle.pack_query_4bit(q[i]))[:dim]
            assert np.array_equal(prepared[i], want), (bits, i)

"""The register-query kernel's split loop with its progress-ordered wave priority (mfma_wide.hip, kOptFlat), launch by
launch through fsgpu_lab_scan_stage against the plain reference of tests/scan_stage_ref.py.

A wave of the split loop lowers its own priority as it advances through a tile and takes the append excursion at the highest level.
Priority moves WHEN a wave's instructions issue and nothing else, so every launch must report exactly what the stage contract says,
and exactly what the same launch reports with the levels switched off (FSGPU_WIDE_PRIO=off: a child process of this file, the switch
is read once per process).  The shapes are the smallest at which the levels, the barrier and the DMA issue points can go wrong:
int8 rows of 384 and 256 dimensions (6 and 4 k-steps), four query tiles per wave, two 512-query groups in one launch with 700 real
queries (the last group ragged, padded with +inf thresholds), 8 walkers per group side by side (16 blocks) and 8 blocks sequential,
5,197 rows (8 x 5 tiles of 128 rows + 77: a partial last tile and a partial pair) and 4,096 rows (exactly four tiles per walker), both
directions, with and without the live / allow bitmaps.

Stage 2 (thresholded main pass): about 1 % of the (query, row) pairs pass; query 3 lets 30 % through, so that its lists overflow into
the spill area and excursions happen at every priority level.  Stage 3 (group maxima): sample groups 4, 5 or 9 groups apart with counts
that leave some blocks an odd number of groups, the last one reaching past the slab's end; the W x 4 entries per query are checked
against the reference's partition of the groups over the blocks.
"""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_stage_ref as S  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QT, GROUPS, WALKERS = 4, 2, 8
NQ_PAD, NQ_REAL = 128 * QT * GROUPS, 700
N_RAGGED, N_WHOLE = WALKERS * 5 * 128 + 77, WALKERS * 4 * 128
SLOTS, SPILL_CAP = 16, 2048
DIMS = (384, 256)
LAYOUTS = ("side_by_side", "sequential")
# stage 3: (group_stride, group_count) per slab.  5,197 rows are 82 groups of 64, the last one partial: 21 groups 4 apart give the 8 blocks
# 2 or 3 groups each; 10 groups 9 apart give them 1 or 2 and end on the partial group 81.  4,096 rows: 16 groups (2 each), 13 groups (1 or 2).
SAMPLES = {N_RAGGED: ((4, 21), (9, 10)), N_WHOLE: ((4, 16), (5, 13))}
INF = np.float32(np.inf)


@functools.lru_cache(maxsize=None)
def data(dim):
    """(rows [N_RAGGED, dim] int8, queries [NQ_PAD, dim] int8 with zero padding queries, live, allow); never changed."""
    rng = np.random.default_rng(4000 + dim)
    rows = rng.integers(-127, 128, (N_RAGGED, dim), dtype=np.int8)
    q = rng.integers(-127, 128, (NQ_PAD, dim), dtype=np.int8)
    q[NQ_REAL:] = 0
    live, allow = rng.random(N_RAGGED) < 0.5, rng.random(N_RAGGED) < 0.5
    return rows, q, live, allow


@functools.lru_cache(maxsize=None)
def scores(dim):
    rows, q, _, _ = data(dim)
    return S.scores_int(rows, q)          # [NQ_PAD, N_RAGGED] int64, exact


@functools.lru_cache(maxsize=None)
def thresholds(dim, nrows, masked):
    """About 1 % of the valid rows pass per query (>= edge for even queries, between two scores for odd ones), 30 % for query 3."""
    _, _, live, allow = data(dim)
    valid = (live & allow)[:nrows] if masked else np.ones(nrows, bool)
    s = np.sort(scores(dim)[:, :nrows][:, valid], axis=1)[:, ::-1]
    nv = s.shape[1]
    kth = s[:, max(1, nv // 100) - 1].astype(np.float64)
    tau = np.where(np.arange(NQ_PAD) % 2 == 1, kth + 0.5, kth).astype(np.float32)
    tau[3] = np.float32(s[3, (nv * 3) // 10])
    tau[NQ_REAL:] = INF
    return tau, valid


def stage_cases(stage):
    """Every launch of a (dim, layout) case of `stage`: (nrows, reverse, masked, group_stride, group_count)."""
    out = []
    for nrows in (N_RAGGED, N_WHOLE):
        for reverse in (0, 1):
            for masked in (False, True):
                for stride, count in (SAMPLES[nrows] if stage == 3 else ((1, 0),)):
                    out.append((nrows, reverse, masked, stride, count))
    return out


@functools.lru_cache(maxsize=None)
def launch(dim, stage, layout, nrows, reverse, masked, stride, count):
    rows, q, live, allow = data(dim)
    tau = thresholds(dim, nrows, masked)[0] if stage == 2 else np.zeros(NQ_PAD, np.float32)
    return S.run_scan(S.REG, QT, stage, 1, dim, rows[:nrows], q, tau, grid=WALKERS, slots=SLOTS if stage == 2 else 0, spill_cap=SPILL_CAP if stage == 2 else 0,
                      groups=GROUPS, live=S.bitmap_words(live[:nrows]) if masked else None, allow=S.bitmap_words(allow[:nrows]) if masked else None,
                      group_stride=stride, group_count=count, reverse=reverse, side_by_side=int(layout == "side_by_side"),
                      want_counts=int(stage == 2 and reverse == 1))


def all_launches():
    for dim in DIMS:
        for stage in (2, 3):
            for layout in LAYOUTS:
                for case in stage_cases(stage):
                    yield (dim, stage, layout) + case


def canonical(out):
    """A launch's output arrays in a form two runs can be compared in: the spill area's ORDER is the order in which blocks won a
    global counter (any two runs differ in it), its content is not; slots past a list's counted length are not written."""
    res = {}
    for name, arr in out.items():
        if name == "spill":
            arr = np.sort(arr, axis=1)
        if name == "cand" and "cand_count" in out:
            arr = np.where(np.arange(arr.shape[2])[None, None, :] < out["cand_count"][:, :, None], arr, S.KEMPTY)
        res[name] = arr
    return res


def key_of(launch_key, name):
    return "_".join(str(int(x) if isinstance(x, (bool, np.bool_)) else x) for x in launch_key) + "__" + name


def _child(path):
    assert os.environ.get("FSGPU_WIDE_PRIO") == "off"
    sys.path.insert(0, ROOT)
    arrays = {}
    for k in all_launches():
        for name, arr in canonical(launch(*k)).items():
            arrays[key_of(k, name)] = arr
    np.savez(path, **arrays)


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    assert _lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    assert "FSGPU_WIDE_PRIO" not in os.environ, "this process must run the levelled loop"


@functools.lru_cache(maxsize=None)
def blocks_of(nrows, rev):
    """The block whose list each row of the 128-row-tile main pass lands in."""
    return np.array([S.row_block(r, S.REG, QT, 2, 384, 1, WALKERS, nrows, 1, 0, rev) for r in range(nrows)])


def group_reverse(layout, reverse, grp):
    return reverse if layout == "side_by_side" else reverse ^ (grp & 1)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_thresholded_main_pass_reports_the_reference_set(dim, layout):
    assert S.tile_rows(S.REG, QT, 2, dim, 1) == 128, "the split loop on 128-row tiles"
    s64 = scores(dim)
    for nrows, reverse, masked, stride, count in stage_cases(2):
        what = (dim, layout, nrows, reverse, masked)
        out = launch(dim, 2, layout, nrows, reverse, masked, stride, count)
        tau, valid = thresholds(dim, nrows, masked)
        taken, lens, spills = S.collect(out, NQ_PAD, WALKERS, SLOTS, SPILL_CAP)
        expect = S.expected_rows(s64[:, :nrows].astype(np.float64), tau, valid)
        npass = sum(len(e) for e in expect[:NQ_REAL])
        share = npass / (NQ_REAL * valid.sum())
        print(f"{what}: {npass} passing pairs ({100 * share:.2f} %), query 3: {len(expect[3])} rows, {int(out['spill_count'][3, 0])} in the spill area")
        assert 0.005 < share < 0.02, (what, "about 1 % of the pairs pass", share)
        assert not np.any(out["overflow"]), (what, "the spill area holds every overflowing entry")
        assert int(out["spill_count"][3, 0]) > 4 * SLOTS, (what, "query 3 must overflow its lists")
        lblk = np.broadcast_to(np.arange(WALKERS)[:, None], (WALKERS, SLOTS))
        for q in range(NQ_PAD):
            got = np.concatenate([out["cand"][q][taken[q]], spills[q]])
            a, rows = S.unpack(got)
            assert int(out["spill_count"][q, 0]) == len(expect[q]) - int(lens[q].sum()), (what, "spill_count = passing pairs - list lengths", q)
            order = np.argsort(rows, kind="stable")
            assert np.array_equal(rows[order], expect[q]), (what, "lists + spill != the expected set", q, np.setxor1d(rows, expect[q])[:8])
            assert np.array_equal(a.view(np.uint32), s64[q, rows].astype(np.float32).view(np.uint32)), (what, "score bits", q)
            blk = blocks_of(nrows, group_reverse(layout, reverse, q // (128 * QT)))
            lrow = S.unpack(out["cand"][q][taken[q]])[1]
            assert np.array_equal(blk[lrow], lblk[taken[q]]), (what, "an entry in another block's list", q)
        assert all(len(e) == 0 for e in expect[NQ_REAL:]), "padding queries report nothing"


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_group_maxima_report_the_reference_partition(dim, layout):
    s64 = scores(dim)
    _, _, live, allow = data(dim)
    G = 128 * QT
    odd = past = 0
    for nrows, reverse, masked, stride, count in stage_cases(3):
        what = (dim, layout, nrows, reverse, masked, stride, count)
        assert stride >= 4
        past += int((count - 1) * stride * 64 + 64 > nrows)
        out = launch(dim, 3, layout, nrows, reverse, masked, stride, count)
        cand = out["cand"]
        assert cand.shape == (NQ_PAD, WALKERS, 4), (what, "W x 4 entries per query")
        assert not np.any(cand == S.UNWRITTEN), (what, "a group-maxima slot was not written")
        valid = (live & allow)[:nrows] if masked else np.ones(nrows, bool)
        for grp in range(GROUPS):
            rev = group_reverse(layout, reverse, grp)
            per_block = np.bincount([S.tile_block(t, WALKERS, count, rev) for t in range(count)], minlength=WALKERS)
            odd += int(np.any(per_block % 2 == 1))
            qs = slice(grp * G, (grp + 1) * G)
            best, have, classes = S.group_maxima_expected(s64[qs, :nrows], valid, nrows, WALKERS, stride, count, rev)
            got = cand[qs]
            assert np.array_equal(got != S.KEMPTY, have), (what, grp, "kEmpty exactly where a class has no valid row")
            a, r = S.unpack(got)
            assert np.array_equal(a[have].view(np.uint32), best[have].astype(np.float32).view(np.uint32)), (what, grp, "group maxima")
            for b in range(WALKERS):
                for fk in range(4):
                    qh = np.flatnonzero(have[:, b, fk])
                    g = r[qh, b, fk] - fk * 4
                    assert np.all(np.isin(g, classes[(b, fk)])), (what, grp, "the reported group is not in the block's class", b, fk)
                    lanes = g[:, None] + np.array([fk * 4 + i for i in range(4)] + [16 + fk * 4 + i for i in range(4)])[None, :]
                    sc = np.where(valid[lanes], s64[grp * G + qh][np.arange(len(qh))[:, None], lanes], np.iinfo(np.int64).min)
                    assert np.array_equal(sc.max(axis=1), best[qh, b, fk]), (what, grp, "the reported group does not attain the score", b, fk)
    assert odd > 0 and past > 0, "the cases must hold a block with an odd number of groups and a group that reaches past the last row"


@pytest.fixture(scope="module")
def flat(tmp_path_factory):
    """Every launch of this file with the priority levels off, from a fresh process."""
    path = str(tmp_path_factory.mktemp("wide_prio") / "off.npz")
    env = dict(os.environ, FSGPU_WIDE_PRIO="off")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("stage", (2, 3))
def test_priority_levels_change_no_output(flat, stage):
    n = 0
    for k in all_launches():
        if k[1] != stage:
            continue
        for name, arr in canonical(launch(*k)).items():
            assert np.array_equal(arr, flat[key_of(k, name)]), (k, name, "differs from the launch without priority levels")
            n += 1
    assert n > 0


if __name__ == "__main__":
    _child(sys.argv[1])

"""The register-query main pass on 128-row tiles, synchronised per ring slot instead of at a block barrier (mfma_wide.hip, kOptBarrier;
DESIGN 3.1e), launch by launch through fsgpu_lab_scan_stage against the plain reference of tests/scan_stage_ref.py and against the
same launch with the block barrier (FSGPU_WIDE_SYNC=barrier: a child process of this file, the switch is read once per process).

A query belongs to one wave and that wave's tile order is fixed, so for the same grid the (query, block) lists, their lengths, the spill
counters and the overflow flags of the two forms must be byte-identical (the ORDER of a query's spill area is the order in which blocks
won a global counter and differs between any two runs; its content does not).  What the slot counters can get wrong is a wave reading a
tile before all of it has landed, or a slot refilled under a wave that still reads it: the launches therefore run long enough for the
three-slot ring to wrap twice, with thresholds that let about one score per tile through (waves stay level) and with thresholds that let
dozens through (many append excursions: waves drift as far apart as the counters allow).

Shapes: int8 rows of 384 and 256 bytes (6 and 4 k-steps), four query tiles per wave; 512 queries (one group) and 1,024 (two groups, side
by side and one after the other); grids of 8 and 24 walkers; 128 (7 grid) + 77 rows — seven rounds, a ragged last round and a tile that
crosses the slab's end — and 128 x 3 + 5 rows (fewer tiles than slots + 1); both directions; live / allow bitmaps with 30 % of the bits
cleared each.  One 2,048-row launch with thresholds of -inf: every row passes for every query, every list fills, spills and overflows.
One end-to-end case: search_batched against the exact search_batch on 200,000 x 384 with 160 queries, rows and f32 bits.
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
QT = 4
G = 128 * QT                       # queries per group
DIMS = (384, 256)
GRIDS = (8, 24)
LAYOUTS = ("one_group", "side_by_side", "sequential")
SLOTS, SPILL_CAP = 16, 2048
N_MAX = 128 * 7 * max(GRIDS) + 77
N_FEW = 128 * 3 + 5
N_ALL, SPILL_CAP_ALL = 2048, 1024   # the -inf launch: 2,048 passing rows per query against 8 x 16 list slots + 1,024 spill entries
E2E_ROWS, E2E_QUERIES, K = 200_000, 160, 10


def rows_of(grid):
    return 128 * 7 * grid + 77


def nq_of(layout):
    return G if layout == "one_group" else 2 * G


@functools.lru_cache(maxsize=None)
def data(dim):
    """(rows [N_MAX, dim] int8, queries [2 G, dim] int8, live, allow: 30 % of the bits cleared each); never changed.  Every launch scans
    a prefix of the rows with a prefix of the queries."""
    rng = np.random.default_rng(7100 + dim)
    rows = rng.integers(-127, 128, (N_MAX, dim), dtype=np.int8)
    q = rng.integers(-127, 128, (2 * G, dim), dtype=np.int8)
    live, allow = rng.random(N_MAX) >= 0.3, rng.random(N_MAX) >= 0.3
    return rows, q, live, allow


@functools.lru_cache(maxsize=None)
def scores(dim):
    rows, q, _, _ = data(dim)
    return S.scores_int(rows, q).astype(np.int32)          # [2 G, N_MAX], exact (|score| <= 384 x 127 x 127)


@functools.lru_cache(maxsize=None)
def best_scores(dim, nrows, masked):
    """Per query the 64 best scores among the valid rows of the first nrows, best first."""
    _, _, live, allow = data(dim)
    valid = (live & allow)[:nrows] if masked else np.ones(nrows, bool)
    s = scores(dim)[:, :nrows][:, valid]
    top = -np.partition(-s, 63, axis=1)[:, :64]
    return np.sort(top, axis=1)[:, ::-1], valid


def thresholds(dim, nrows, masked, dense):
    """sparse: about one passing score per (tile, 512-query group) — every step-th query of a group lets its best row through, the others
    nothing.  dense: dozens per tile — every query lets its k best rows through, k = 48 tiles / 512 (at least 1)."""
    top, valid = best_scores(dim, nrows, masked)
    ntiles = (nrows + 127) // 128
    if dense:
        k = max(1, -(-48 * ntiles // G))
        tau = top[:, k - 1].astype(np.float32)
    else:
        step = max(1, G // ntiles)
        tau = np.where((np.arange(2 * G) % G) % step == 0, top[:, 0], top[:, 0] + 1).astype(np.float32)
    return tau, valid


def launches_of(grid):
    """(nrows, reverse, masked, dense) of every launch of a (dim, layout, grid) case."""
    n = rows_of(grid)
    return ((n, 0, False, False), (n, 1, True, False), (n, 0, True, True), (n, 1, False, True), (N_FEW, 0, True, True), (N_FEW, 1, False, False))


@functools.lru_cache(maxsize=None)
def launch(dim, layout, grid, nrows, reverse, masked, dense):
    rows, q, live, allow = data(dim)
    nq = nq_of(layout)
    tau = thresholds(dim, nrows, masked, dense)[0][:nq]
    return S.run_scan(S.REG, QT, 2, 1, dim, rows[:nrows], q[:nq], tau, grid=grid, slots=SLOTS, spill_cap=SPILL_CAP, groups=nq // G,
                      live=S.bitmap_words(live[:nrows]) if masked else None, allow=S.bitmap_words(allow[:nrows]) if masked else None,
                      reverse=reverse, side_by_side=int(layout == "side_by_side"), want_counts=int(reverse == 1))


@functools.lru_cache(maxsize=None)
def launch_all(dim):
    """Thresholds of -inf on 2,048 rows, one group on 8 walkers: everything passes."""
    rows, q, _, _ = data(dim)
    return S.run_scan(S.REG, QT, 2, 1, dim, rows[:N_ALL], q[:G], np.full(G, -np.inf, np.float32), grid=8, slots=SLOTS, spill_cap=SPILL_CAP_ALL,
                      groups=1, reverse=0, side_by_side=0, want_counts=1)


def all_launches():
    for dim in DIMS:
        for layout in LAYOUTS:
            for grid in GRIDS:
                for case in launches_of(grid):
                    yield (dim, layout, grid) + case


def canonical(out):
    """A launch's output arrays in the form two runs are compared in: the spill area sorted per query, list slots past the counted
    length (not written) blanked."""
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


@functools.lru_cache(maxsize=None)
def e2e_corpus():
    rng = np.random.default_rng(7200)
    cent = rng.standard_normal((64, 384)).astype(np.float32)
    cent /= np.linalg.norm(cent, axis=1, keepdims=True)
    rows = cent[rng.integers(0, 64, E2E_ROWS)] + (0.7 / np.sqrt(384)) * rng.standard_normal((E2E_ROWS, 384)).astype(np.float32)
    q = rows[rng.integers(0, E2E_ROWS, E2E_QUERIES)] + (0.5 / np.sqrt(384)) * rng.standard_normal((E2E_QUERIES, 384)).astype(np.float32)
    return rows.astype(np.float16), q.astype(np.float32)


def last_kernel():
    from frankensearch_amd import _lib
    return _lib.lib().fsgpu_last_main_pass_kernel().decode()


def e2e_batched():
    import frankensearch_amd as fa
    slab, q = e2e_corpus()
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16))
    rows, sc, counts, _ = idx.search_batched(q, K)
    kernel = last_kernel()
    idx.close()
    return rows, np.ascontiguousarray(sc, np.float32).view(np.uint32), counts, kernel


def _child(path):
    assert os.environ.get("FSGPU_WIDE_SYNC") == "barrier"
    sys.path.insert(0, ROOT)
    arrays = {}
    for k in all_launches():
        for name, arr in canonical(launch(*k)).items():
            arrays[key_of(k, name)] = arr
    assert last_kernel().endswith(", 3, 62>"), last_kernel()
    for dim in DIMS:
        for name, arr in canonical(launch_all(dim)).items():
            arrays[f"all_{dim}__{name}"] = arr
    rows, sc, counts, kernel = e2e_batched()
    assert kernel.endswith(", 3, 62>"), kernel
    arrays.update(e2e_rows=rows, e2e_scores=sc, e2e_counts=counts)
    np.savez(path, **arrays)


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    assert _lib.lib().fsgpu_device_count() >= 1, "no GPU visible"
    assert "FSGPU_WIDE_SYNC" not in os.environ, "this process must run the slot-synchronised loop"


@pytest.fixture(scope="module")
def barrier(tmp_path_factory):
    """Every launch of this file with the block barrier per tile, from a fresh process."""
    path = str(tmp_path_factory.mktemp("wide_sync") / "barrier.npz")
    env = dict(os.environ, FSGPU_WIDE_SYNC="barrier")
    res = subprocess.run([sys.executable, os.path.abspath(__file__), path], env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    return np.load(path)


@functools.lru_cache(maxsize=None)
def tile_blocks(grid, nrows, rev):
    """The block whose list each row lands in."""
    ntiles = (nrows + 127) // 128
    per_tile = np.array([S.tile_block(t, grid, ntiles, rev) for t in range(ntiles)])
    return per_tile[np.arange(nrows) // 128]


def reported_pairs(out, nq, grid, spill_cap):
    """Every (query, row, score bits, block or -1 for the spill area) a launch reported, sorted by (query, row)."""
    taken, lens, spills = S.collect(out, nq, grid, SLOTS, spill_cap)
    qi, bi, _ = np.nonzero(taken)
    a, r = S.unpack(out["cand"][taken])
    sq = np.concatenate([np.full(len(s), q) for q, s in enumerate(spills)] + [np.zeros(0, np.int64)]).astype(np.int64)
    sa, sr = S.unpack(np.concatenate(list(spills) + [np.zeros(0, np.uint64)]))
    q_all, r_all = np.concatenate([qi, sq]), np.concatenate([r, sr])
    bits_all = np.concatenate([a.view(np.uint32), sa.view(np.uint32)])
    b_all = np.concatenate([bi, np.full(len(sq), -1)])
    order = np.lexsort((r_all, q_all))
    return q_all[order], r_all[order], bits_all[order], b_all[order], lens


@pytest.mark.parametrize("grid", GRIDS)
@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("dim", DIMS)
def test_slot_synchronised_main_pass_reports_the_reference_set(dim, layout, grid):
    assert S.tile_rows(S.REG, QT, 2, dim, 1) == 128, "the split loop on 128-row tiles"
    nq = nq_of(layout)
    for nrows, reverse, masked, dense in launches_of(grid):
        what = (dim, layout, grid, nrows, reverse, masked, dense)
        out = launch(dim, layout, grid, nrows, reverse, masked, dense)
        assert last_kernel().endswith(", 3, 30>"), last_kernel()
        tau, valid = thresholds(dim, nrows, masked, dense)
        s = scores(dim)[:nq, :nrows]
        want = valid[None, :] & (s >= tau[:nq, None])       # (integer scores against integer-valued f32 thresholds: exact)
        wq, wr = np.nonzero(want)
        ntiles = (nrows + 127) // 128
        groups = nq // G
        print(f"{what}: {len(wq)} passing pairs, {len(wq) / (ntiles * groups):.1f} per tile and group")
        if dense:
            assert len(wq) >= 24 * ntiles * groups, (what, "dozens of passing scores per tile")
        else:
            assert 0.5 * ntiles * groups <= len(wq) <= 3 * ntiles * groups, (what, "about one passing score per tile")
        gq, gr, gbits, gblk, lens = reported_pairs(out, nq, grid, SPILL_CAP)
        assert not np.any(out["overflow"]), (what, "the spill area holds every overflowing entry")
        assert np.array_equal(gq, wq) and np.array_equal(gr, wr), (what, "lists + spill != the expected set")
        assert np.array_equal(gbits, s[wq, wr].astype(np.float32).view(np.uint32)), (what, "score bits")
        assert np.array_equal(out["spill_count"][:, 0], want.sum(axis=1) - lens.sum(axis=1)), (what, "spill_count = passing pairs - list lengths")
        for grp in range(groups):
            rev = reverse if layout != "sequential" else reverse ^ (grp & 1)
            blk = tile_blocks(grid, nrows, rev)
            m = (gq // G == grp) & (gblk >= 0)
            assert np.array_equal(blk[gr[m]], gblk[m]), (what, "an entry in another block's list", grp)


@pytest.mark.parametrize("dim", DIMS)
def test_thresholds_of_minus_infinity_fill_spill_and_overflow_every_list(dim, barrier):
    out = launch_all(dim)
    taken, lens, spills = S.collect(out, G, 8, SLOTS, SPILL_CAP_ALL)
    assert np.all(lens == SLOTS), "every list is full"
    assert np.all(out["overflow"] == 1), "every query overflows its spill area"
    assert np.all(out["spill_count"][:, 0] == N_ALL - 8 * SLOTS), "spill_count = passing pairs - list lengths"
    s = scores(dim)[:G, :N_ALL]
    blk = tile_blocks(8, N_ALL, 0)
    for q in range(G):
        a, r = S.unpack(out["cand"][q])
        assert np.array_equal(blk[r], np.broadcast_to(np.arange(8)[:, None], (8, SLOTS))), (q, "an entry in another block's list")
        sa, sr = S.unpack(spills[q])
        assert len(sr) == SPILL_CAP_ALL, (q, "the spill area is full")
        both = np.concatenate([r.ravel(), sr])
        assert len(np.unique(both)) == len(both) and both.max() < N_ALL, (q, "a row reported twice or a row that does not exist")
        assert np.array_equal(np.concatenate([a.ravel(), sa]).view(np.uint32), s[q, both].astype(np.float32).view(np.uint32)), (q, "score bits")
    for name in ("cand", "cand_count", "spill_count", "overflow"):
        assert np.array_equal(out[name], barrier[f"all_{dim}__{name}"]), (dim, name, "differs from the launch with the block barrier")


def test_slot_synchronisation_changes_no_output(barrier):
    n = 0
    for k in all_launches():
        for name, arr in canonical(launch(*k)).items():
            assert np.array_equal(arr, barrier[key_of(k, name)]), (k, name, "differs from the launch with the block barrier")
            n += 1
    assert n > 0


def test_batched_search_equals_the_exact_search(barrier):
    import frankensearch_amd as fa
    slab, q = e2e_corpus()
    rows, sc, counts, kernel = e2e_batched()
    assert kernel.endswith(", 3, 30>"), kernel
    idx = fa.VectorIndex.from_slab(slab.view(np.uint16))
    er, es, ec = idx.search_batch(q, K, exact=True)
    idx.close()
    assert np.all(ec == K) and np.array_equal(counts, ec)
    assert np.array_equal(rows, er)
    assert np.array_equal(sc, np.ascontiguousarray(es, np.float32).view(np.uint32))
    assert np.array_equal(rows, barrier["e2e_rows"]) and np.array_equal(sc, barrier["e2e_scores"]) and np.array_equal(counts, barrier["e2e_counts"])


if __name__ == "__main__":
    _child(sys.argv[1])

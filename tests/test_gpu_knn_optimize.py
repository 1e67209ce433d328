"""fsgpu_knn_graph_optimize (knn_optimize_kernels.hip, vector_index_knn_optimize.cpp) against tests/knn_optimize_ref.py:
the device's table equals the reference's byte for byte at the smallest shapes at which each kernel can go wrong — every width class
of the detour kernel's loads, one and many blocks, rows past 2^16 (a third sort digit varies, several sort tiles), a run of reverse
candidates far longer than a list, tables that are wrong in every way — and on tables the index built itself.  test_knn_optimize_
contract.py shows, without a GPU, that each rule of the contract reaches the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ann_ref as R  # noqa: E402
import knn_optimize_ref as ref  # noqa: E402
from ann_cases import bits, score_table  # noqa: E402

pytestmark = pytest.mark.gpu
PAD = ref.PAD
STAT_NAMES = ("rows", "forward_edges", "reverse_edges", "zero_in_degree_before", "zero_in_degree_after", "max_detour_count")


@pytest.fixture(scope="module")
def fa():
    import frankensearch_amd as fa_mod
    from frankensearch_amd.build import build

    build()
    return fa_mod


def bare_index(fa, n, row_base=0):
    """The optimisation reads no vector: any slab of n rows supplies the device, the stream, record_count and row_base."""
    return fa.VectorIndex.from_slab(np.zeros((n, 8), dtype=np.uint16), row_base=row_base)


def local_table(rng, n, w, row_base, spread=None):
    """Neighbours from a window around the row, so that lists share entries and detours exist; lists of differing length."""
    spread = spread or max(2 * w, 4)
    off = rng.integers(1, spread + 1, (n, w)) * rng.choice([-1, 1], (n, w))
    t = (np.arange(n)[:, None] + off) % n + row_base
    lens = rng.integers(0, w + 1, n)
    lens[rng.random(n) < 0.7] = w
    t[np.arange(w)[None, :] >= lens[:, None]] = PAD
    return t.astype(np.uint32)


def hostile_table(rng, n, w, row_base):
    """Pads in mid-list, ids past the index and below row_base, self-loops, repeated ids, all-pad rows, short clean lists."""
    t = local_table(rng, n, w, row_base, spread=max(w // 2, 2)).astype(np.int64)   # a narrow window: many repeats
    kind = rng.random((n, w))
    t[kind < 0.06] = PAD
    t[(kind >= 0.06) & (kind < 0.12)] = row_base + n + rng.integers(0, 5)
    t[(kind >= 0.12) & (kind < 0.14)] = 0xFFFFFFFE
    if row_base:
        t[(kind >= 0.14) & (kind < 0.18)] = rng.integers(0, row_base)
    loops = (kind >= 0.18) & (kind < 0.24)
    t[loops] = (np.arange(n)[:, None] + row_base + np.zeros((1, w), np.int64))[loops]
    t[rng.random(n) < 0.1] = PAD
    return t.astype(np.uint32)


def assert_device_is_reference(fa, table, d, row_base, what):
    n = table.shape[0]
    idx = bare_index(fa, n, row_base)
    want_stats = {}
    want = ref.optimize(table, d, row_base, stats=want_stats)
    got, stats = idx.optimize_knn_graph(table, d, want_stats=True)
    again = idx.optimize_knn_graph(table, d)
    differing = int((got != want).any(axis=1).sum())
    print(f"{what}: N {n} w {table.shape[1]} d {d} row_base {row_base}: rows differing {differing}, stats {stats}")
    assert got.dtype == np.uint32 and got.shape == want.shape
    assert differing == 0, (what, np.flatnonzero((got != want).any(axis=1))[:5])
    assert got.tobytes() == want.tobytes() == again.tobytes()
    assert {k: stats[k] for k in STAT_NAMES} == {k: want_stats[k] for k in STAT_NAMES}
    assert stats["device_ms"] > 0.0
    return got


def degrees(w):
    return sorted({1, (w + 1) // 2, w})


@pytest.mark.parametrize("w", [1, 2, 7, 16, 33, 63, 64])
@pytest.mark.parametrize("row_base", [0, 1_000_003])
def test_widths_and_degrees(fa, w, row_base):
    """Every width class (one column, below a 16-byte unit, odd, whole units, past 32, one below and at the wave) at 257 rows — more
    than one block, a last block with one row — and every degree class of it."""
    rng = np.random.default_rng(100 + w)
    table = local_table(rng, 257, w, row_base)
    for d in degrees(w):
        assert_device_is_reference(fa, table, d, row_base, "widths")


@pytest.mark.parametrize("n", [1, 2, 17])
@pytest.mark.parametrize("row_base", [0, 1_000_003])
def test_tiny_indexes(fa, n, row_base):
    rng = np.random.default_rng(n)
    for w in (1, 7, 16):
        table = local_table(rng, n, w, row_base)
        for d in degrees(w):
            assert_device_is_reference(fa, table, d, row_base, "tiny")


@pytest.mark.parametrize("w, d, row_base", [(16, 8, 0), (16, 16, 1_000_003), (33, 17, 0)])
def test_4096_rows(fa, w, d, row_base):
    table = local_table(np.random.default_rng(4096 + w), 4096, w, row_base)
    assert_device_is_reference(fa, table, d, row_base, "4096 rows")


@pytest.mark.parametrize("d, row_base", [(4, 0), (8, 1_000_003)])
def test_rows_past_two_to_the_sixteenth(fa, d, row_base):
    """70,001 rows at w = 8: row numbers past 2^16 make a third digit of both key halves vary, and a round's keys fill several sort
    tiles.  Half the lists point far away (targets and sources in different tiles), half stay near."""
    rng = np.random.default_rng(70001)
    n = 70001
    table = local_table(rng, n, 8, row_base).astype(np.int64)
    far = rng.random(n) < 0.5
    table[far] = np.where(table[far] == PAD, PAD, rng.integers(0, n, (int(far.sum()), 8)) + row_base)
    assert_device_is_reference(fa, table.astype(np.uint32), d, row_base, "70,001 rows")


@pytest.mark.parametrize("n, w, d", [(4096, 8, 4), (4096, 7, 7), (70001, 4, 3)])
def test_hub_rows(fa, n, w, d):
    """Every row lists row 5 at column 0: a run of N - 1 reverse candidates of rank 0, cut at d in source order.  A second hub (row
    11) stands at the last rank of every list, so its run arrives when its list is part full and straddles the cut."""
    rng = np.random.default_rng(n + w)
    table = local_table(rng, n, w, 0, spread=4 * w)
    table[table == PAD] = (np.argwhere(table == PAD)[:, 0] + 1) % n   # full lists: the last column is the last rank
    table[:, 0] = 5
    table[:, w - 1] = 11
    table[11, 0] = 3   # (row 11's own list: something other than the hub at rank 0)
    got = assert_device_is_reference(fa, table, d, 0, "hub")
    h = (d + 1) // 2
    fwd, _ = ref.forward_lists(table, d)
    assert [int(g) for g in got[5, h:d]] == [x for x in range(n) if x != 5 and x not in fwd[5][:h]][:d - h]


@pytest.mark.parametrize("n, w, d, row_base", [(17, 7, 4, 0), (300, 16, 16, 1_000_003), (1000, 33, 17, 7), (513, 64, 64, 0), (4096, 12, 6, 1_000_003)])
def test_hostile_tables(fa, n, w, d, row_base):
    rng = np.random.default_rng(n * 100 + w)
    table = hostile_table(rng, n, w, row_base)
    table[n // 2] = PAD
    table[n // 3, :] = PAD
    table[n // 3, 0] = (n // 3 + 1) % n + row_base   # a clean list of one entry (or none, at n = 1)
    got = assert_device_is_reference(fa, table, d, row_base, "hostile")
    ids = got[got != PAD].astype(np.int64) - row_base
    assert ((ids >= 0) & (ids < n)).all()


# ---- tables the index built ------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def corpus():
    return ref.structured_corpus(seed=2, n=4096, nq=100)


@pytest.mark.parametrize("f32, tombstones", [(False, False), (True, False), (False, True)])
def test_built_table(fa, oracle, corpus, f32, tombstones):
    """build_knn_graph(32) at 4,096 rows, optimised to 16 columns: the reference's bytes; build_ann(32, optimize=16) answers as the
    reference search does over the reference's optimisation of that table, and not as build_ann(16) does."""
    x, queries = corpus
    rng = np.random.default_rng(5)
    live = None
    if tombstones:
        live = np.ones(len(x), dtype=bool)
        live[rng.choice(len(x), size=len(x) // 10, replace=False)] = False
    slab = (x * (1.0 + 1e-4 * rng.standard_normal(x.shape))).astype(np.float32) if f32 else x.astype(np.float16)
    make = fa.VectorIndex.from_slab_f32 if f32 else fa.VectorIndex.from_slab
    idx = make(slab, live=live)
    table = idx.build_knn_graph(32)
    want_stats = {}
    want = ref.optimize(table, 16, stats=want_stats)
    got, stats = idx.optimize_knn_graph(table, 16, want_stats=True)
    print(f"built table f32 {f32} tombstones {tombstones}: {stats}")
    assert got.tobytes() == want.tobytes()
    assert {k: stats[k] for k in STAT_NAMES} == {k: want_stats[k] for k in STAT_NAMES}
    if not tombstones:
        assert stats["zero_in_degree_before"] > 0 and stats["zero_in_degree_after"] == 0

    cfg = dict(n_entry=16, expand=4, max_iters=64)
    ann = idx.build_ann(32, optimize=16, **cfg)
    plain = idx.build_ann(16, **cfg)
    scores = score_table(oracle, slab.view(np.uint16) if not f32 else slab, queries, f32, 0)
    rows, sc, counts, flags = ann.search_batched(queries, 10, 16)
    prows = plain.search_batched(queries, 10, 16)[0]
    for i in range(len(queries)):
        wr, ws, wc, _, _ = R.search(scores[i], live, want, 10, 16, **cfg)
        assert flags[i] == 0 and counts[i] == wc and (rows[i, :wc] == wr).all() and (bits(sc[i, :wc]) == bits(ws)).all(), i
    assert (rows != prows).any()
    # the default is the exact table, searched as before
    assert plain.search_batched(queries, 10, 16)[0].tobytes() == fa.AnnIndex(idx, idx.build_knn_graph(16), fa.AnnConfig(**cfg)) \
        .search_batched(queries, 10, 16)[0].tobytes()
    for i in range(0, len(queries), 10):
        wr, _, wc, _, _ = R.search(scores[i], live, table[:, :16], 10, 16, **cfg)
        assert (prows[i, :wc] == wr).all()


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------

def test_refusals_write_nothing(fa):
    from frankensearch_amd import _lib
    idx = bare_index(fa, 100)
    L = _lib.lib()
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    table = local_table(np.random.default_rng(1), 100, 16, 0)
    wide = local_table(np.random.default_rng(1), 100, 65, 0)
    cases = {"graph_len below record_count": (table[:99], 99, 16, 8), "graph_len above record_count": (table, 101, 16, 8),
             "degree 0": (table, 100, 16, 0), "degree above the width": (table, 100, 16, 17), "width above 64": (wide, 100, 65, 8)}
    for why, (t, glen, w, d) in cases.items():
        t = np.ascontiguousarray(t)
        out = np.full((101, 64), 0x12345678, dtype=np.uint32)
        st = _lib.KnnOptimizeStats()
        st.rows = 77
        assert L.fsgpu_knn_graph_optimize(idx._h, ptr(t), glen, w, d, ptr(out), ctypes.addressof(st)) == _lib.ERR_INVALID_CONFIG, why
        assert (out == 0x12345678).all() and st.rows == 77, why
    out = np.full((100, 8), 0x12345678, dtype=np.uint32)
    assert L.fsgpu_knn_graph_optimize(idx._h, None, 100, 16, 8, ptr(out), None) == _lib.ERR_INVALID_CONFIG
    assert L.fsgpu_knn_graph_optimize(idx._h, ptr(table), 100, 16, 8, None, None) == _lib.ERR_INVALID_CONFIG
    assert (out == 0x12345678).all()
    with pytest.raises(fa.InvalidConfig):
        idx.optimize_knn_graph(table, 17)
    with pytest.raises(fa.InvalidConfig):
        idx.optimize_knn_graph(table[:50], 8)
    # an empty index: OK, nothing done
    empty = fa.VectorIndex.from_slab(np.zeros((0, 8), dtype=np.uint16))
    assert empty.optimize_knn_graph(np.zeros((0, 16), dtype=np.uint32), 8).shape == (0, 8)


def test_refused_while_a_begun_search_is_outstanding(fa):
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    rng = np.random.default_rng(3)
    idx = fa.VectorIndex.from_slab(rng.standard_normal((1000, 64)).astype(np.float16))
    table = local_table(rng, 1000, 16, 0)
    dev = torch.device("cuda", 0)
    be = GpuShardBackend(idx, dev, batched=True)
    q = torch.from_numpy(rng.standard_normal((8, 64)).astype(np.float32)).to(dev)
    _, ticket = be.scan_begin(q, 10, packed=False)
    with pytest.raises(fa.InvalidConfig):
        idx.optimize_knn_graph(table, 8)
    be.scan_end(ticket)
    assert idx.optimize_knn_graph(table, 8).tobytes() == ref.optimize(table, 8).tobytes()

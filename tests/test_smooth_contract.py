"""The neighbour smoothing at the C ABI (fsgpu_neighbor_smooth) against the reference's inline tests and a numpy restatement, and
the error paths of the k-NN graph build that need no device.  No GPU."""
from __future__ import annotations

import ctypes as C

import numpy as np
import pytest

from tests import smooth_ref as R

F32 = np.float32
PAD = R.PAD


def _fa():
    import frankensearch_amd as fa
    return fa


def bits(xs):
    return np.asarray(xs, dtype=F32).view(np.uint32)


def graph_of(docs, edges, width=4):
    """Doc strings -> rows (their position in `docs`), (from, to) pairs -> a padded row table in insertion order."""
    row = {d: i for i, d in enumerate(docs)}
    g = np.full((len(docs), width), PAD, dtype=np.uint32)
    fill = [0] * len(docs)
    for a, b in edges:
        g[row[a], fill[row[a]]] = row[b]
        fill[row[a]] += 1
    return g, row


def hits_of(row, pairs):
    return [(d, s, row[d]) for d, s in pairs]


def score_of(out, doc):
    return [s for d, s, _ in out if d == doc][0]


# ---- smooth.rs:300-560, with their literals ----

def test_alpha_zero_is_identity():
    fa = _fa()
    g, row = graph_of(["a", "b"], [("a", "b"), ("b", "a")])
    hits = hits_of(row, [("a", 0.9), ("b", 0.5)])
    out = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.0))
    assert [(d, i) for d, _, i in out] == [(d, i) for d, _, i in hits]
    assert np.array_equal(bits([s for _, s, _ in out]), bits([0.9, 0.5]))


def test_ranked_identity_is_byte_identical():
    fa = _fa()
    g, row = graph_of(["a", "b", "c"], [("a", "b"), ("b", "a"), ("b", "c")])
    hits = hits_of(row, [("a", 0.9), ("b", 0.5), ("c", 0.4)])
    for cfg, graph in ((fa.SmoothConfig(alpha=0.0), g), (fa.SmoothConfig(), np.zeros((0, 4), np.uint32)), (fa.SmoothConfig(), None),
                       (fa.SmoothConfig(m=0), g), (fa.SmoothConfig(alpha=float("nan")), g), (fa.SmoothConfig(alpha=-1.0), g)):
        out = fa.neighbor_smooth_ranked(hits, graph, cfg)
        assert [d for d, _, _ in out] == ["a", "b", "c"]
        assert np.array_equal(bits([s for _, s, _ in out]), bits([0.9, 0.5, 0.4]))
    # *out_applied reports the identity
    from frankensearch_amd.fusion import _pack
    arr, _keep = _pack(hits)
    applied = C.c_uint8(7)
    cfg = fa.SmoothConfig(alpha=0.0)._c()
    assert fa._lib.lib().fsgpu_neighbor_smooth(arr, 3, g.ctypes.data, 3, 4, C.addressof(cfg), 1, C.byref(applied)) == 0
    assert applied.value == 0
    cfg = fa.SmoothConfig()._c()
    assert fa._lib.lib().fsgpu_neighbor_smooth(arr, 3, g.ctypes.data, 3, 4, C.addressof(cfg), 1, C.byref(applied)) == 0
    assert applied.value == 1
    assert fa._lib.lib().fsgpu_neighbor_smooth(arr, 0, g.ctypes.data, 3, 4, C.addressof(cfg), 1, C.byref(applied)) == 0
    assert applied.value == 0


def test_ranked_reorders_a_promoted_doc_where_plain_smooth_does_not():
    fa = _fa()
    g, row = graph_of(["a", "b", "c", "d"], [("c", "a"), ("a", "c"), ("c", "d"), ("d", "c")])
    hits = hits_of(row, [("a", 0.90), ("b", 0.60), ("c", 0.55)])
    cfg = fa.SmoothConfig(alpha=0.5, m=10, mutual=False)
    plain = fa.neighbor_smooth(hits, g, cfg)
    ranked = fa.neighbor_smooth_ranked(hits, g, cfg)
    assert bits([score_of(plain, "c")])[0] == bits([score_of(ranked, "c")])[0]
    assert score_of(ranked, "c") > score_of(plain, "b")
    assert [d for d, _, _ in plain].index("c") == 2
    assert [d for d, _, _ in ranked].index("c") == 1
    for (d0, s0, _), (d1, s1, _) in zip(ranked, ranked[1:]):
        assert R.total_key(s0) > R.total_key(s1) or (R.total_key(s0) == R.total_key(s1) and d0 <= d1)


def test_empty_graph_is_identity():
    fa = _fa()
    hits = [("a", 0.9, 0), ("b", 0.5, 1)]
    out = fa.neighbor_smooth(hits, np.zeros((0, 3), np.uint32), fa.SmoothConfig())
    assert [d for d, _, _ in out] == ["a", "b"] and np.array_equal(bits([s for _, s, _ in out]), bits([0.9, 0.5]))


def test_hand_computed_mean():
    fa = _fa()
    g, row = graph_of(["d", "a", "b"], [("d", "a"), ("d", "b")])
    out = fa.neighbor_smooth(hits_of(row, [("d", 0.2), ("a", 0.9), ("b", 0.7)]), g, fa.SmoothConfig(alpha=0.5, m=10))
    assert abs(score_of(out, "d") - 0.5) < 1e-6


def test_cluster_rescues_below_threshold_relevant():
    fa = _fa()
    g, row = graph_of(["a", "b", "c", "d", "b_iso", "far"], [("d", "a"), ("d", "b"), ("d", "c"), ("b_iso", "far")])
    hits = hits_of(row, [("a", 0.92), ("b", 0.90), ("c", 0.88), ("d", 0.30), ("b_iso", 0.40)])
    out = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.3, m=10))
    assert score_of(out, "d") > score_of(out, "b_iso")
    assert abs(score_of(out, "b_iso") - 0.40) < 1e-6


def test_isolated_doc_unchanged():
    fa = _fa()
    g, row = graph_of(["x", "y", "not_in_pool"], [("x", "not_in_pool")])
    out = fa.neighbor_smooth(hits_of(row, [("x", 0.55), ("y", 0.80)]), g, fa.SmoothConfig())
    assert abs(score_of(out, "x") - 0.55) < 1e-6


def test_mutual_knn_ignores_one_way_edges():
    fa = _fa()
    g, row = graph_of(["d", "a"], [("d", "a")])
    hits = hits_of(row, [("d", 0.20), ("a", 0.90)])
    non_mutual = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.5, m=10, mutual=False))
    assert abs(score_of(non_mutual, "d") - 0.55) < 1e-6
    mutual = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.5, m=10, mutual=True))
    assert abs(score_of(mutual, "d") - 0.20) < 1e-6


def test_m_cap_limits_neighbors():
    fa = _fa()
    g, row = graph_of(["d", "a", "b", "c"], [("d", "a"), ("d", "b"), ("d", "c")])
    out = fa.neighbor_smooth(hits_of(row, [("d", 0.2), ("a", 0.9), ("b", 0.6), ("c", 0.0)]), g, fa.SmoothConfig(alpha=1.0, m=2))
    assert abs(score_of(out, "d") - 0.75) < 1e-6


def test_preserves_index_and_docs():
    fa = _fa()
    g = np.full((8, 2), PAD, dtype=np.uint32)
    g[7, 0], g[3, 0] = 3, 7
    out = fa.neighbor_smooth([("a", 0.5, 7), ("b", 0.9, 3)], g, fa.SmoothConfig())
    assert len(out) == 2 and out[0][2] == 7 and out[0][0] == "a" and out[1][2] == 3


# ---- searcher.rs:6615-6650 and :6738-6790, at the pool ----

def test_hubness_is_applied_before_smoothing_so_hubs_do_not_leak_into_neighbor_means():
    """correct_phase1_pool with both corrections: the penalty without its sort, the smoothing, ONE sort.  doc-1 borrows from the
    de-hubbed doc-4: 0.5 * 0.0 + 0.5 * (1.0 - 0.5 * 1.0) = 0.25, not 0.5."""
    fa = _fa()
    g = np.full((5, 1), PAD, dtype=np.uint32)
    g[1, 0] = 4
    hits = [("doc-0", 1.0, 0), ("doc-4", 1.0, 4), ("doc-1", 0.0, 1)]
    demoted = fa.apply_hubness_penalty(hits, [0.0, 0.0, 0.0, 0.0, 1.0], fa.HubnessConfig(beta=0.5), resort=False)
    out = fa.neighbor_smooth_ranked(demoted, g, fa.SmoothConfig(alpha=0.5))
    assert abs(score_of(out, "doc-1") - 0.25) < 1e-6
    assert abs(score_of(out, "doc-4") - 0.5) < 1e-6
    assert abs(score_of(out, "doc-0") - 1.0) < 1e-6
    assert [d for d, _, _ in out] == ["doc-0", "doc-4", "doc-1"]
    wrong = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.5))   # smoothing first would give 0.5
    assert abs(score_of(wrong, "doc-1") - 0.5) < 1e-6


def test_smoothing_is_inert_by_default_and_promotes_a_graph_neighbor_of_a_top_hit():
    fa = _fa()
    g = np.full((8, 1), PAD, dtype=np.uint32)
    g[7, 0] = 0
    hits = [("doc-0", 1.0, 0)] + [(f"doc-{i}", 0.0, i) for i in range(1, 8)]
    base = fa.neighbor_smooth_ranked(hits, g, fa.SmoothConfig(alpha=0.0))
    assert [d for d, _, _ in base] == [d for d, _, _ in hits]
    assert np.array_equal(bits([s for _, s, _ in base]), bits([s for _, s, _ in hits]))
    rank = lambda out, doc: [d for d, _, _ in out].index(doc)
    assert rank(base, "doc-7") > rank(base, "doc-2")
    out = fa.neighbor_smooth_ranked(hits, g, fa.SmoothConfig(alpha=0.5))
    assert rank(out, "doc-7") < rank(out, "doc-2") and rank(out, "doc-0") == 0
    assert abs(score_of(out, "doc-7") - 0.5) < 1e-6


# ---- fsgpu_neighbor_smooth == the numpy restatement, bit for bit ----

def _random_case(seed):
    rng = np.random.default_rng(seed)
    glen = int(rng.integers(1, 400))
    width = int(rng.integers(1, 64))
    g = rng.integers(0, glen, size=(glen, width), dtype=np.uint32)
    # lists with pads: a random tail of some lists; a pad in mid-list (what lies behind it must be ignored); a few rows past the table
    for r in rng.choice(glen, size=max(glen // 3, 1), replace=False):
        g[r, int(rng.integers(0, width + 1)):] = PAD
    for r in rng.choice(glen, size=max(glen // 10, 1), replace=False):
        g[r, int(rng.integers(0, width))] = PAD
    for r in rng.choice(glen, size=max(glen // 10, 1), replace=False):
        g[r, int(rng.integers(0, width))] = glen + int(rng.integers(0, 5))
    n = [0, 1, 2, 300][seed % 4] if seed % 10 == 0 else int(rng.integers(0, 301))
    idx = rng.integers(0, glen + 6, size=n).astype(np.int64)       # some rows past graph_len
    if n >= 3:
        idx[n - 1] = idx[0]                                         # a duplicated row: its last occurrence is the pool's score
    if n >= 5:
        idx[1] = 0xFFFFFFFF
    scores = rng.uniform(-1, 1, size=n).astype(F32)
    if n >= 8 and seed % 3 == 0:
        scores[rng.integers(0, n)] = np.nan
        scores[rng.integers(0, n)] = np.inf
        scores[rng.integers(0, n)] = -np.inf
    if n >= 4:
        scores[2] = scores[3]                                       # an exact tie: the doc id decides
    hits = [(f"d{int(rng.integers(0, 50)):02d}-{i}", scores[i], int(idx[i])) for i in range(n)]
    m = [max(width - 1, 1), width, width + 3, 1, 10][seed % 5]     # below, at and above the width
    alpha = [1e-30, 0.3, 1.0, 2.0, float("nan"), -1.0][seed % 6]
    return hits, g, alpha, m, bool(seed % 2)


@pytest.mark.parametrize("block", range(4))
def test_abi_equals_the_restatement_bit_for_bit(block):
    fa = _fa()
    for seed in range(block * 50, block * 50 + 50):   # 200 cases in all
        hits, g, alpha, m, mutual = _random_case(seed)
        cfg = fa.SmoothConfig(alpha=alpha, m=m, mutual=mutual)
        for resort in (False, True):
            got = (fa.neighbor_smooth_ranked if resort else fa.neighbor_smooth)(hits, g, cfg)
            want = R.neighbor_smooth(hits, g, alpha, m, mutual, resort=resort)
            assert [(d, i) for d, _, i in got] == [(d, i & 0xFFFFFFFF) for d, _, i in want], (seed, resort)
            assert np.array_equal(bits([s for _, s, _ in got]), bits([s for _, s, _ in want])), (seed, resort)


def test_mutual_mode_equals_the_direct_definition():
    """For each counted neighbour nb of a hit on row r: nb is among the first min(m, width) entries of r's list before any pad, is
    in the pool, and a linear scan of ALL of nb's stored columns finds r.  And every such neighbour is counted."""
    fa = _fa()
    seen = 0
    for seed in range(1, 60, 2):
        hits, g, _alpha, m, _ = _random_case(seed)
        counted = []
        want = R.neighbor_smooth(hits, g, 0.3, m, True, counted=counted)
        got = fa.neighbor_smooth(hits, g, fa.SmoothConfig(alpha=0.3, m=m, mutual=True))
        assert np.array_equal(bits([s for _, s, _ in got]), bits([s for _, s, _ in want])), seed
        pool = {i for _, _, i in hits}
        glen, width = g.shape
        for (_, _, row), used in zip(hits, counted):
            direct = []
            if row < glen:
                for e in range(min(m, width)):
                    nb = int(g[row, e])
                    if nb == PAD:
                        break
                    if nb in pool and nb < glen and row in [int(x) for x in g[nb].tolist()]:
                        direct.append(nb)
            assert used == direct, (seed, row)
            seen += len(used)
    assert seen > 0, "no mutual edge in any case: nothing was checked"
    # the reciprocity looks at every stored column, not the first m: a <-> b where a sits in b's LAST column
    g = np.full((3, 4), PAD, dtype=np.uint32)
    g[0, 0] = 1
    g[1] = [2, 2, 2, 0]
    out = fa.neighbor_smooth([("a", 0.2, 0), ("b", 0.8, 1)], g, fa.SmoothConfig(alpha=0.5, m=1, mutual=True))
    assert abs(score_of(out, "a") - 0.5) < 1e-6


def test_knn_from_topk_self_rule():
    assert R.knn_from_topk([5, 3, 9, 1], 3, 3) == [5, 9, 1]
    assert R.knn_from_topk([5, 3, 9, 1], 7, 3) == [5, 3, 9]          # self absent: the last entry goes
    assert R.knn_from_topk([3], 3, 2) == [PAD, PAD]
    assert R.knn_from_topk([4, 3], 3, 3) == [4, PAD, PAD]


# ---- errors that need no device ----

def test_config_defaults_and_reserved_words():
    fa = _fa()
    from frankensearch_amd.smooth import _SmoothConfig
    L = fa._lib.lib()
    c = _SmoothConfig()
    assert L.fsgpu_smooth_config_default(C.addressof(c)) == 0
    assert c.alpha == F32(0.3) and c.m == 10 and c.mutual == 0 and list(c.reserved) == [0] * 5
    assert L.fsgpu_smooth_config_default(None) == fa._lib.ERR_NULL_ARGUMENT
    from frankensearch_amd.fusion import _pack
    arr, _keep = _pack([("a", 0.5, 0)])
    g = np.zeros((1, 1), np.uint32)
    for word in range(5):
        bad = _SmoothConfig(0.3, 10, 0)
        bad.reserved[word] = 1
        assert L.fsgpu_neighbor_smooth(arr, 1, g.ctypes.data, 1, 1, C.addressof(bad), 1, None) == fa._lib.ERR_INVALID_CONFIG
    assert L.fsgpu_neighbor_smooth(None, 1, g.ctypes.data, 1, 1, None, 1, None) == fa._lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_neighbor_smooth(arr, 1, g.ctypes.data, 1, 1, None, 1, None) == 0   # NULL config: the defaults


def test_knn_graph_build_errors_without_a_device():
    """m is checked before anything else, then the device.  The range check needs a handle, and a handle needs a device: it is
    asserted here where one is visible and in tests/test_gpu_knn_graph.py."""
    import torch
    fa = _fa()
    L = fa._lib.lib()
    out = np.zeros(64, np.uint32)
    for build in (L.fsgpu_index_build_knn_graph, L.fsgpu_sharded_build_knn_graph):
        for m in (0, 64):
            assert build(None, 0, 1, m, out.ctypes.data, None) == fa._lib.ERR_INVALID_CONFIG
        if not torch.cuda.is_available():
            assert build(None, 0, 1, 10, out.ctypes.data, None) == fa._lib.ERR_NO_DEVICE
            assert "no HIP device" in fa._lib.last_error()
        else:
            assert build(None, 0, 1, 10, out.ctypes.data, None) == fa._lib.ERR_NULL_ARGUMENT
    if torch.cuda.is_available():
        idx = fa.VectorIndex.from_slab(np.ones((5, 8), np.float16), device=0)
        for first, n in ((0, 6), (5, 1), (6, 0), (2 ** 40, 1)):
            assert L.fsgpu_index_build_knn_graph(idx._h, first, n, 3, out.ctypes.data, None) == fa._lib.ERR_INVALID_CONFIG
        assert L.fsgpu_index_build_knn_graph(idx._h, 5, 0, 3, None, None) == 0   # n_rows == 0: OK, nothing done

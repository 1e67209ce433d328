"""The graph optimisation of include/fsgpu.h (fsgpu_knn_graph_optimize) as tests/knn_optimize_ref.py states it, without
a GPU: it makes the beam search of tests/ann_ref.py find its neighbours on a corpus with structure, every rule of the contract
reaches the table, and the output is well formed on hostile tables."""
import numpy as np
import pytest

import ann_ref
import knn_optimize_ref as ref

PAD = ref.PAD


@pytest.fixture(scope="module")
def corpus():
    x, q = ref.structured_corpus(seed=2, n=4096, nq=100)
    table = ann_ref.knn_table(x, 32)
    scores = (q @ x.T).astype(np.float32)
    exact = np.argsort(-scores, axis=1, kind="stable")[:, :10]
    return dict(table=table, optimised=ref.optimize(table, 16), scores=scores, exact=exact)


def recall(graph, scores, exact, ef):
    got = []
    for s, e in zip(scores, exact):
        rows, _, count, _, _ = ann_ref.search(s, None, graph, 10, ef, n_entry=16, expand=4, max_iters=64)
        got.append(ann_ref.recall_at_k_of(rows[:count], e))
    return float(np.mean(got))


@pytest.mark.parametrize("ef", [16, 128])
def test_optimised_table_is_found_by_the_beam_search_where_the_exact_prefix_is_not(corpus, ef):
    before = recall(np.ascontiguousarray(corpus["table"][:, :16]), corpus["scores"], corpus["exact"], ef)
    after = recall(corpus["optimised"], corpus["scores"], corpus["exact"], ef)
    print(f"ef {ef}: recall@10 exact prefix {before:.3f}, optimised {after:.3f}")
    assert after >= before + 0.2


def test_optimised_table_reaches_every_row(corpus):
    before = ref.zero_in_degree(corpus["table"][:, :16])
    after = ref.zero_in_degree(corpus["optimised"])
    print(f"in-degree-0 rows: exact prefix {before}, optimised {after}")
    assert before > 0 and after == 0


# ---- every rule, broken alone, gives another table on a case that aims at it ----------------------------------------------------

def table_of(lists, w):
    t = np.full((len(lists), w), PAD, dtype=np.uint32)
    for x, lst in enumerate(lists):
        t[x, :len(lst)] = lst
    return t


def test_rule_ties_go_to_the_lower_rank():
    # no list holds a neighbour's neighbour: every count is 0 and the order is the rank's alone
    t = table_of([[1, 2, 3], [4, 5, 6], [4, 5, 6], [4, 5, 6], [], [], []], 3)
    good = ref.optimize(t, 2)
    assert good[0].tolist() == [1, 2]
    assert not np.array_equal(good, ref.optimize(t, 2, ties_desc=True))


def test_rule_the_detour_hop_ranks_strictly_above_the_edge():
    # row 0: rank 1 (row 2) is met in row 1's list at column 1 — p = i, no detour; with p <= i it would fall behind rank 2
    t = table_of([[1, 2, 3], [4, 2, 5], [4, 5, 6], [4, 5, 6], [], [], []], 3)
    good = ref.optimize(t, 2)
    assert good[0, 0] == 1 and 2 in good[0].tolist()
    assert not np.array_equal(good, ref.optimize(t, 2, p_le_i=True))
    # ... and at column 0 it is one: rank 1 falls behind rank 2
    t2 = table_of([[1, 2, 3], [2, 4, 5], [4, 5, 6], [4, 5, 6], [], [], []], 3)
    clean, counts = ref.detour_counts(t2)
    assert counts[0] == [0, 1, 0]
    assert ref.forward_lists(t2, 3)[0][0] == [1, 3, 2]


def test_rule_reverse_candidates_in_source_order():
    # rows 1 .. 5 all list row 0 first: its reverse candidates are cut at d in ascending source order
    t = table_of([[6]] + [[0, 6]] * 5 + [[]], 2)
    good = ref.optimize(t, 2)
    assert good[0].tolist() == [6, 1]
    assert not np.array_equal(good, ref.optimize(t, 2, reverse_desc=True))


def test_rule_the_merge_lists_a_row_once():
    # rows 0 and 1 list each other: the reverse candidate is already there
    t = table_of([[1, 2], [0, 2], [3], []], 2)
    good = ref.optimize(t, 2)
    assert good[0].tolist() == [1, 2] and good[1].tolist() == [0, 2]
    assert not np.array_equal(good, ref.optimize(t, 2, no_dedup=True))


def test_rule_no_pad_before_an_entry():
    # row 3 has one forward entry and one reverse candidate: dense from column 0 in a list of 4
    t = table_of([[3, 1, 2, 4], [0, 2, 4, 5], [0, 1, 4, 5], [5], [], []], 4)
    good = ref.optimize(t, 4)
    row = good[3].tolist()
    assert row[:2] == [5, 0] and row[2:] == [PAD, PAD]
    assert not np.array_equal(good, ref.optimize(t, 4, pad_mid=True))


# ---- invariants on hostile tables --------------------------------------------------------------------------------------------------

def hostile_table(rng, n, w, row_base):
    """Ids inside and outside the table, below row_base, self-loops, repeats, pads in mid-list, all-pad rows."""
    t = rng.integers(0, n, (n, w)).astype(np.int64) + row_base
    kind = rng.random((n, w))
    t[kind < 0.08] = PAD
    t[(kind >= 0.08) & (kind < 0.14)] = row_base + n + rng.integers(0, 5)
    if row_base:
        t[(kind >= 0.14) & (kind < 0.18)] = rng.integers(0, row_base)
    loops = (kind >= 0.18) & (kind < 0.24)
    t[loops] = (np.arange(n)[:, None] + row_base + np.zeros((1, w), np.int64))[loops]
    t[rng.random(n) < 0.1] = PAD
    return t.astype(np.uint32)


@pytest.mark.parametrize("n, w, d, row_base", [(1, 1, 1, 0), (2, 2, 1, 0), (17, 7, 4, 0), (61, 16, 16, 1000003), (200, 33, 17, 7), (97, 64, 64, 0)])
def test_output_is_well_formed_on_hostile_tables(n, w, d, row_base):
    rng = np.random.default_rng(n * 1000 + w)
    t = hostile_table(rng, n, w, row_base)
    stats = {}
    out = ref.optimize(t, d, row_base, stats=stats)
    fwd, _ = ref.forward_lists(t, d, row_base)
    h = (d + 1) // 2
    assert out.shape == (n, d) and out.dtype == np.uint32
    entries = 0
    for x in range(n):
        row = out[x].tolist()
        count = row.index(PAD) if PAD in row else d
        assert all(g == PAD for g in row[count:]), "entries are dense before the pads"
        local = [g - row_base for g in row[:count]]
        assert all(0 <= r < n for r in local)
        assert x not in local
        assert len(set(local)) == len(local)
        assert local[:min(h, len(fwd[x]))] == fwd[x][:h]
        entries += count
    assert stats["forward_edges"] + stats["reverse_edges"] == entries and stats["rows"] == n

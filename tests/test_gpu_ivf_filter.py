"""GPU checks of the IVF index's int8 list filter (fsgpu_ivf_set_list_filter).  Stage by stage through
fsgpu_lab_ivf_filter_stage against tests/ivf_filter_ref.py with no tolerance anywhere — the ordered copy's bytes, every integer
score, t, m, counts, flags and the candidate arrays — and end to end on one handle: filter on == filter off (== tests/ivf_ref.py) in
rows, score bits, counts, flags and every fsgpu_ivf_stats field but launches and device_ms."""
import ctypes as C
import functools
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import ivf_cases as CS  # noqa: E402
import ivf_filter_cases as FC  # noqa: E402
import ivf_filter_ref as FR  # noqa: E402
import ivf_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
bits = R.bits
UNWRITTEN = 0xA5A5A5A5
STAT_FIELDS = ("index_size", "dimension", "nlist", "nprobe", "k_requested", "queries", "approximate", "underfilled",
               "empty_despite_indexed_points", "lists_probed", "rows_scored")


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


class _StageArgs(C.Structure):
    _fields_ = [("queries", C.c_void_p), ("nq", C.c_uint32), ("query_len", C.c_uint32), ("k", C.c_uint32), ("nprobe", C.c_uint32),
                ("slots_cap", C.c_uint32), ("reserved0", C.c_uint32), ("scores_cap", C.c_uint64), ("out_ordered", C.c_void_p),
                ("out_delta", C.c_void_p), ("out_ran", C.c_void_p), ("out_nslots", C.c_void_p), ("out_slot_query", C.c_void_p),
                ("out_slot_list", C.c_void_p), ("out_slot_offset", C.c_void_p), ("out_scores", C.c_void_p), ("out_t", C.c_void_p),
                ("out_m", C.c_void_p), ("out_count", C.c_void_p), ("out_flag", C.c_void_p), ("out_cand", C.c_void_p)]


def stage(fa, ivf, queries, k, nprobe):
    """fsgpu_lab_ivf_filter_stage -> dict of its outputs, cut to the call's slots."""
    q = np.ascontiguousarray(queries, dtype=F32)
    nq, dim = q.shape
    offsets, _ = ivf.lists()
    cap = nq * nprobe
    scores_cap = cap * int(np.diff(offsets.astype(np.int64)).max())
    o = dict(ordered=np.full((int(offsets[-1]), dim), 99, np.int8), delta=np.zeros(nq, F32), ran=np.zeros(1, np.uint32),
             nslots=np.zeros(1, np.uint32), slot_query=np.zeros(cap, np.uint32), slot_list=np.zeros(cap, np.uint32),
             slot_offset=np.zeros(cap + 1, np.uint64), scores=np.zeros(max(scores_cap, 1), np.int32), t=np.zeros(cap, np.int32),
             m=np.zeros(cap, np.int64), count=np.zeros(cap, np.uint32), flag=np.zeros(cap, np.uint32),
             cand=np.zeros((cap, FC.SLOT_CAP), np.uint32))
    a = _StageArgs(q.ctypes.data, nq, dim, k, nprobe, cap, 0, scores_cap, *[o[n].ctypes.data for n in (
        "ordered", "delta", "ran", "nslots", "slot_query", "slot_list", "slot_offset", "scores", "t", "m", "count", "flag", "cand")])
    rc = fa._lib.lib().fsgpu_lab_ivf_filter_stage(ivf._h, C.addressof(a))
    assert rc == 0, fa._lib.last_error()
    n = int(o["nslots"][0])
    for name in ("slot_query", "slot_list", "t", "m", "count", "flag", "cand"):
        o[name] = o[name][:n]
    o["slot_offset"] = o["slot_offset"][:n + 1]
    o["ran"], o["nslots"] = int(o["ran"][0]), n
    return o


def check_stage(oracle, fa, idx, ivf, queries, k, nprobe, live=None, hreduce=0, what=""):
    """The stage's outputs against the restatement, from the index's own codes and bound.  -> (the outputs, slots that overflowed)"""
    q = np.ascontiguousarray(queries, dtype=F32)
    delta, _, _, qi8, slab_i8 = idx.int8_filter_bound(q, want_slab=True)
    offsets, rows = ivf.lists()
    n = slab_i8.shape[0]
    live_b = np.ones(n, dtype=bool) if live is None else np.asarray(live, dtype=bool)
    index = R.Index(ivf.centroids(), offsets, rows, live_b, hreduce, 0, 0)
    o = stage(fa, ivf, q, k, nprobe)
    assert (o["ordered"] == slab_i8[rows]).all(), f"{what}: the ordered copy is not filter_i8[list_rows]"
    assert (bits(o["delta"]) == bits(delta)).all(), f"{what}: the handle's bound is not the index's"
    assert o["ran"] == int((delta >= 0).any()), what
    if not o["ran"]:
        return o, 0
    want_slots = FR.slots(index, [R.probe(oracle, index, x, nprobe) for x in q])
    assert list(zip(o["slot_query"].tolist(), o["slot_list"].tolist())) == want_slots, f"{what}: slot table"
    overflowed = 0
    for s, (qi, l) in enumerate(want_slots):
        lr = index.list_rows(l)
        got = o["scores"][int(o["slot_offset"][s]):int(o["slot_offset"][s + 1])]
        want = FR.scores(qi8[qi], slab_i8, lr, live_b)
        assert got.size == lr.size and (got.astype(np.int64) == want).all(), f"{what}: slot {s} (query {qi}, list {l}): integer scores"
        if delta[qi] >= 0:
            t, m, count, flag, cand = FR.select(want, lr, k, delta[qi], FC.SLOT_CAP)
        else:
            t, m, count, flag, cand = FR.DEAD, 0, 0, FR.UNCERTIFIED, np.zeros(0, np.uint32)
        assert (int(o["t"][s]), int(o["m"][s]), int(o["count"][s]), int(o["flag"][s])) == (t, m, count, flag), f"{what}: slot {s} (query {qi}, list {l})"
        keep = min(count, FC.SLOT_CAP)
        assert (o["cand"][s, :keep] == cand[:keep]).all(), f"{what}: slot {s}: candidates"
        assert (o["cand"][s, keep:] == UNWRITTEN).all(), f"{what}: slot {s}: written past its candidates"
        overflowed += flag == FR.OVERFLOW
    return o, overflowed


def same_answers(a, b, what):
    (ra, sa, ca, fa_), (rb, sb, cb, fb) = a, b
    assert (ca == cb).all() and (fa_ == fb).all(), f"{what}: counts or flags differ"
    for i in range(len(ca)):
        c = int(ca[i])
        assert (ra[i, :c] == rb[i, :c]).all() and (bits(sa[i, :c]) == bits(sb[i, :c])).all(), f"{what}: query {i} differs"


def on_equals_off(ivf, queries, k, nprobe, what=""):
    """-> (the answer, the filter's stats, the stats with the filter on)."""
    ivf.set_list_filter(False)
    off = ivf.search_batched(queries, k, nprobe)
    st_off, f_off = ivf.stats, ivf.filter_stats()
    assert f_off.mode == 0 and (f_off.queries_filtered, f_off.slots_filtered, f_off.rows_filtered, f_off.calls_above_k_cap) == (0, 0, 0, 0)
    ivf.set_list_filter(True)
    assert ivf.list_filter
    on = ivf.search_batched(queries, k, nprobe)
    st_on, f_on = ivf.stats, ivf.filter_stats()
    same_answers(on, off, f"{what} k {k} nprobe {nprobe}")
    for name in STAT_FIELDS:
        assert getattr(st_on, name) == getattr(st_off, name), (what, name)
    assert (f_on.mode, f_on.slot_cap, f_on.k_cap) == (1, FC.SLOT_CAP, FC.K_CAP)
    assert f_on.queries_filtered + f_on.queries_uncertified == (len(queries) if k <= FC.K_CAP else 0)
    return on, f_on, st_on


def assert_reference(oracle, slab, want, queries, answer, k, nprobe, live=None, row_base=0):
    rows, sc, counts, flags = answer
    for i, q in enumerate(queries):
        wr, ws, wf = R.search(oracle, slab, want, q, k, nprobe, live_now=live, row_base=row_base)
        assert counts[i] == wr.size and flags[i] == wf and (rows[i, :wr.size] == wr).all() and (bits(sc[i, :wr.size]) == bits(ws)).all(), i


# ---- 1. stage by stage ----

@pytest.mark.parametrize("dim", [64, 72, 200, 384])
def test_every_stage_is_the_restatement(oracle, dim):
    """64: one k-step; 72: a zero-padded pitch of 128; 200: three k-steps and a padded fourth; 384: six.  One row in seven is dead."""
    fa = _fa()
    slab = CS.normal_rows(dim, 1500, dim)
    live = CS.one_in_seven_dead(1500)
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(12, iters=1, list_filter=True)
    queries = CS.noisy_queries(slab, 20, dim)
    for k, nprobe in ((10, 3), (1, 12), (64, 1)):
        check_stage(oracle, fa, idx, ivf, queries, k, nprobe, live=live, what=f"dim {dim} k {k} nprobe {nprobe}")
    f = ivf.filter_stats()
    pitch = (dim + 63) // 64 * 64
    lens = np.diff(ivf.lists()[0].astype(np.int64))
    assert (f.rotated, f.copy_bytes) == (0, int(FR.round_up(lens, 16).sum()) * pitch) and f.build_ms > 0


@functools.lru_cache(maxsize=None)
def contract_case(which):
    from oracle import oracle
    oracle.build()
    fa = _fa()
    slab, queries, live = FC.clustered(oracle, nq=200) if which == "clustered" else FC.hashmix(oracle)
    c = FC.CLUSTERED if which == "clustered" else FC.HASHMIX
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"], list_filter=True)
    return fa, idx, ivf, slab, queries, live, R.build(oracle, slab, c["nlist"], c["iters"], live=live)


def test_the_stages_on_the_clustered_corpus_keep_a_few_rows_a_slot(oracle):
    fa, idx, ivf, slab, queries, live, want = contract_case("clustered")
    c = FC.CLUSTERED
    o, overflowed = check_stage(oracle, fa, idx, ivf, queries[:c["nq"]], c["k"], c["nprobe"], what="clustered")
    assert o["nslots"] == 240 and overflowed == 0 and int(o["count"].max()) <= 29 and not o["flag"].any()


def test_the_stages_on_the_hashmix_rows_overflow(oracle):
    fa, idx, ivf, slab, queries, live, want = contract_case("hashmix")
    c = FC.HASHMIX
    o, overflowed = check_stage(oracle, fa, idx, ivf, queries, c["k"], c["nprobe"], live=live, what="hashmix")
    assert o["nslots"] == 76 and overflowed >= 1 and (o["flag"] == 0).any()


# ---- 2. end to end ----

@pytest.mark.parametrize("hreduce", [0, 1, 2])
def test_filter_on_is_filter_off_is_the_reference_on_the_clustered_corpus(oracle, hreduce):
    fa, _, _, slab, queries, live, want0 = contract_case("clustered")
    c = FC.CLUSTERED
    idx = fa.VectorIndex.from_slab(slab)
    idx.set_hreduce(hreduce)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"])
    want = want0 if hreduce == 0 else R.build(oracle, slab, c["nlist"], c["iters"], hreduce=hreduce)
    nq = len(queries)
    for k in (1, 10, 64, 65):
        for nprobe in (1, 5, c["nlist"]):
            on, f, st = on_equals_off(ivf, queries, k, nprobe, what=f"clustered hreduce {hreduce}")
            if k == 65:   # above the cap: the whole call by the unfiltered path
                assert (f.calls_above_k_cap, f.queries_filtered, f.slots_filtered, f.rows_filtered) == (1, 0, 0, 0)
                assert f.rows_rescored == st.rows_scored   # every exact dot was made
                continue
            assert (f.calls_above_k_cap, f.queries_filtered, f.queries_uncertified, f.scratch_ranges) == (0, nq, 0, 1)
            assert 0 < f.slots_filtered <= nq * nprobe and f.rows_filtered == st.rows_scored
            if k == 10 and nprobe <= 8:   # the path proven taken: no overflow, and fewer exact dots than rows in the probed lists
                assert f.slots_overflowed == 0 and f.rows_rescored < f.rows_filtered
                print(f"clustered hreduce {hreduce} k {k} nprobe {nprobe}: {f.rows_rescored} exact dots for {f.rows_filtered} int8 dots; "
                      f"filter {f.filter_ms:.3f} ms, select {f.select_ms:.3f} ms, rescore {f.rescore_ms:.3f} ms")
            if k == 10 and nprobe == 5:
                assert_reference(oracle, slab, want, queries[:40], tuple(x[:40] for x in on), k, nprobe)


def test_an_answer_does_not_depend_on_the_batch_the_position_or_the_form(oracle):
    import torch
    fa, idx, ivf, slab, queries, live, want = contract_case("clustered")
    k, nprobe = 10, 5
    ivf.set_list_filter(True)
    batch = np.concatenate([queries, queries[:57]])   # 257 queries
    rows, sc, counts, flags = ivf.search_batched(batch, k, nprobe)
    assert ivf.filter_stats().queries_filtered == 257
    perm = np.random.default_rng(3).permutation(257)
    same_answers(ivf.search_batched(batch[perm], k, nprobe), (rows[perm], sc[perm], counts[perm], flags[perm]), "permuted")
    for pos in (0, 130, 256):   # the batch of one: the coarse step's other form too
        r1, s1, flag = ivf.search(batch[pos], k, nprobe)
        assert ivf.filter_stats().queries_filtered == 1
        assert flag == flags[pos] and r1.size == counts[pos] and (r1 == rows[pos, :r1.size]).all() and (bits(s1) == bits(sc[pos, :r1.size])).all()
    dq = torch.from_numpy(batch).cuda()
    drows = torch.full((257, k), 7, dtype=torch.int32, device="cuda")
    dsc = torch.zeros((257, k), dtype=torch.float32, device="cuda")
    dcounts = torch.zeros(257, dtype=torch.int32, device="cuda")
    dflags = torch.full((257,), 9, dtype=torch.int32, device="cuda")
    torch.cuda.synchronize()
    ivf.search_batched_device(dq.data_ptr(), 257, k, nprobe, drows.data_ptr(), dsc.data_ptr(), dcounts.data_ptr(), dflags.data_ptr())
    assert ivf.filter_stats().queries_filtered == 257
    same_answers((drows.cpu().numpy().view(np.uint32), dsc.cpu().numpy(), dcounts.cpu().numpy().view(np.uint32),
                  dflags.cpu().numpy().view(np.uint32)), (rows, sc, counts, flags), "device queries")


def test_overflowed_slots_are_scanned_whole_and_the_answers_stand(oracle):
    fa, idx, ivf, slab, queries, live, want = contract_case("hashmix")
    c = FC.HASHMIX
    for k, nprobe in ((c["k"], c["nprobe"]), (1, 5), (64, 16)):
        on, f, st = on_equals_off(ivf, queries, k, nprobe, what="hashmix")
        if k == c["k"]:
            assert f.slots_overflowed > 0 and f.slots_filtered == 76 and f.queries_filtered == len(queries)
            assert f.rows_rescored <= f.rows_filtered   # (the margin is wider than the spread: the slots that pass keep nearly all their rows)
            assert_reference(oracle, slab, want, queries, on, k, nprobe, live=live)


def test_more_single_member_groups_than_one_scan_launch_takes(oracle):
    """1,100 queries x 64 probed lists are 70,400 slots, each a group of the second plan: the gather scan runs in two launches of up to
    65,535 groups."""
    fa, idx, ivf, slab, queries, live, want = contract_case("clustered")
    rng = np.random.default_rng(11)
    q = (np.tile(queries, (6, 1))[:1100] + 0.02 * rng.standard_normal((1100, slab.shape[1]))).astype(F32)
    on, f, st = on_equals_off(ivf, q, 10, 64, what="70,400 slots")
    assert f.slots_filtered > 65535 and f.queries_filtered == 1100 and f.rows_rescored < f.rows_filtered
    assert st.launches == 1 + 2 + 2   # the coarse step, the score and the selection, two scan launches
    er, es, ec = idx.search_batch(q[:50], 10, exact=True)   # every list probed: the exact search
    same_answers(tuple(x[:50] for x in on), (er, es, ec, np.zeros(50, np.uint32)), "nprobe = nlist")


# ---- 3. tile edges ----

def test_lists_and_member_counts_at_the_tile_edges(oracle):
    """Lists of 1, 15, 16, 17, k, k + 1 and 513 rows and an empty one (the caller's centroids); 1, 15, 16, 17 and 33 member queries on
    the 513-row list — alone (nprobe 1) and beside every other list (nprobe = nlist)."""
    fa = _fa()
    slab, init, lens = FC.edge_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(len(lens), iters=0, init_centroids=init, list_filter=True)
    assert np.diff(ivf.lists()[0].astype(np.int64)).tolist() == list(lens)
    want = R.build(oracle, slab, len(lens), 0, init=init)
    for members in FC.MEMBER_COUNTS:
        q = FC.edge_queries(slab.shape[1], members)
        for nprobe in (1, len(lens)):
            o, _ = check_stage(oracle, fa, idx, ivf, q, 10, nprobe, what=f"{members} members nprobe {nprobe}")
            assert o["nslots"] == members * (1 if nprobe == 1 else len(lens) - 1)   # the empty list owns no slot
            on, f, _ = on_equals_off(ivf, q, 10, nprobe, what=f"edges, {members} members")
            assert f.queries_filtered == members
    assert_reference(oracle, slab, want, q, on, 10, len(lens))


def test_twin_centroids_and_lists_of_equal_rows(oracle):
    """duplicate_corpus: every list holds 50 copies of one row — every integer score of a slot ties, all 50 are candidates — and the
    higher twin of every centroid pair is empty; duplicate_queries probe a pair of twins."""
    fa = _fa()
    slab, nlist = CS.duplicate_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(nlist, iters=0, list_filter=True)
    q = CS.duplicate_queries()
    o, _ = check_stage(oracle, fa, idx, ivf, q, 10, 2, what="duplicates")
    assert o["nslots"] == 64 and (o["count"] == 50).all()
    on, f, st = on_equals_off(ivf, q, 10, 2, what="duplicates")
    assert f.rows_rescored == f.rows_filtered == st.rows_scored == 64 * 50


# ---- 4. liveness and certification ----

def test_deletes_made_after_the_filter_was_enabled_are_honoured(oracle):
    fa, _, _, slab, queries, live0, want = contract_case("hashmix")
    c = FC.HASHMIX
    idx = fa.VectorIndex.from_slab(slab, live=live0)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"], list_filter=True)
    on_equals_off(ivf, queries, 10, 2, what="before the deletes")
    live = live0.copy()
    live[::3] = False
    idx.set_live(live)
    check_stage(oracle, fa, idx, ivf, queries[:12], 10, 2, live=live, what="after the deletes")
    on, f, _ = on_equals_off(ivf, queries, 10, 2, what="after the deletes")
    assert_reference(oracle, slab, want, queries, on, 10, 2, live=live)


def test_a_wholly_dead_probed_list_falls_back_as_it_does_today(oracle):
    fa = _fa()
    slab, init, query, short = CS.underfill_corpus()
    n = slab.shape[0]
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(2, iters=1, init_centroids=init, list_filter=True)
    queries = np.stack([query, R.widen(slab[3]), query])
    on, f, st = on_equals_off(ivf, queries, 10, 1, what="short list")
    assert on[3].tolist() == [R.UNDERFILLED, 0, R.UNDERFILLED] and f.slots_filtered == 3
    live = np.ones(n, dtype=bool)
    live[short] = False
    idx.set_live(live)
    o, _ = check_stage(oracle, fa, idx, ivf, queries, 10, 1, live=live, what="dead list")
    assert o["count"].tolist().count(0) == 2   # the two slots of the dead list have no candidate
    on, f, st = on_equals_off(ivf, queries, 10, 1, what="dead list")
    er, es, ec = idx.search_batch(queries, 10, exact=True)
    assert on[3].tolist() == [R.EMPTY, 0, R.EMPTY] and (on[0] == er).all() and (bits(on[1]) == bits(es)).all()
    assert (st.underfilled, st.empty_despite_indexed_points, st.approximate) == (0, 2, 1)


def test_queries_the_bound_does_not_cover_take_the_unfiltered_path_in_the_same_call(oracle):
    fa, _, _, slab, _, live, _ = contract_case("hashmix")
    c = CS.NONFINITE_Q
    idx = fa.VectorIndex.from_slab(slab, live=live)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"], list_filter=True)
    q = CS.nonfinite_queries(slab, c["nq"], c["at"])
    o, _ = check_stage(oracle, fa, idx, ivf, q, c["k"], c["nprobe"], live=live, what="non-finite queries")
    assert sorted(set(o["slot_query"][o["flag"] == FR.UNCERTIFIED].tolist())) == sorted(c["at"])
    on, f, st = on_equals_off(ivf, q, c["k"], c["nprobe"], what="non-finite queries")
    assert (f.queries_uncertified, f.queries_filtered) == (3, c["nq"] - 3)
    assert f.slots_filtered == int((o["flag"] != FR.UNCERTIFIED).sum())


def test_a_slab_the_bound_does_not_cover_filters_nothing(oracle):
    fa = _fa()
    slab, nlist = CS.nonfinite_corpus()
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(nlist, iters=1, list_filter=True)
    q = CS.noisy_queries(slab[100:], 17, 5)
    o, _ = check_stage(oracle, fa, idx, ivf, q, 10, 3, what="NaN slab")
    assert o["ran"] == 0 and (o["delta"] < 0).all()
    on, f, st = on_equals_off(ivf, q, 10, 3, what="NaN slab")
    assert (f.queries_filtered, f.queries_uncertified, f.slots_filtered, f.rows_rescored) == (0, 17, 0, st.rows_scored)


# ---- 5. the rotated copy ----

def test_a_rotated_filter_copy_is_honoured(oracle):
    fa, _, _, slab, queries, live, want = contract_case("clustered")
    c = FC.CLUSTERED
    idx = fa.VectorIndex.from_slab(slab)
    idx.set_filter_rotation(2)   # before first use
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"], list_filter=True)
    o, _ = check_stage(oracle, fa, idx, ivf, queries[:40], c["k"], c["nprobe"], what="rotated")
    on, f, st = on_equals_off(ivf, queries, c["k"], c["nprobe"], what="rotated")
    assert f.rotated == 1 and f.queries_filtered == len(queries) and f.rows_rescored < f.rows_filtered
    assert_reference(oracle, slab, want, queries[:20], tuple(x[:20] for x in on), c["k"], c["nprobe"])
    # the handle's copy is its own: the index may switch its filter afterwards
    idx.set_batched_filter(1)
    same_answers(ivf.search_batched(queries, c["k"], c["nprobe"]), on, "after the index changed its filter")


# ---- 6. the scratch cap, on both sides ----

def test_a_call_above_the_scratch_runs_in_ranges_and_a_tile_above_it_is_scanned_whole(oracle):
    fa, idx, ivf, slab, queries, live, want = contract_case("hashmix")
    L = fa._lib.lib()
    lens = np.diff(ivf.lists()[0].astype(np.int64))
    ivf.set_list_filter(True)
    base = ivf.search_batched(queries, 10, 2)
    f0 = ivf.filter_stats()
    assert (f0.scratch_cap, f0.scratch_ranges, f0.slots_above_scratch) == (FC.SCRATCH_ENTRIES, 1, 0)
    try:
        # the largest list's 16-member tile fits, the call does not: several ranges, nothing above
        cap = int(FR.round_up(lens.max(), 16)) * 16
        assert L.fsgpu_lab_ivf_filter_set_scratch(ivf._h, cap) == 0
        same_answers(ivf.search_batched(queries, 10, 2), base, "ranges")
        f = ivf.filter_stats()
        assert f.scratch_cap == cap and f.scratch_ranges > 1 and f.slots_above_scratch == 0
        assert (f.slots_filtered, f.slots_overflowed, f.rows_filtered, f.rows_rescored) == (f0.slots_filtered, f0.slots_overflowed, f0.rows_filtered, f0.rows_rescored)
        # one entry less: that tile is above the scratch; its slots are scanned whole
        assert L.fsgpu_lab_ivf_filter_set_scratch(ivf._h, int(FR.round_up(lens.max(), 16)) - 1) == 0
        same_answers(ivf.search_batched(queries, 10, 2), base, "above the scratch")
        f = ivf.filter_stats()
        assert f.slots_above_scratch > 0 and f.slots_filtered + f.slots_above_scratch == f0.slots_filtered and f.rows_rescored >= f0.rows_rescored
    finally:
        assert L.fsgpu_lab_ivf_filter_set_scratch(ivf._h, 0) == 0
    same_answers(ivf.search_batched(queries, 10, 2), base, "default scratch")
    assert ivf.filter_stats().scratch_ranges == 1


# ---- 7. the handle ----

def test_the_handle_keeps_its_rules_with_the_filter_on(oracle):
    fa, _, _, slab, queries, live, want = contract_case("clustered")
    c = CS.CERT
    idx = fa.VectorIndex.from_slab(slab)
    ivf = idx.build_ivf(c["nlist"], iters=c["iters"])
    L = fa._lib.lib()
    k = c["k"]
    # certify_nprobe: field for field the filter-off result
    chosen_off, sweep_off = ivf.certify_nprobe(queries, c["candidates"], k, c["target"], c["alpha"])
    st_off = ivf.stats
    ivf.set_list_filter(True)
    chosen_on, sweep_on = ivf.certify_nprobe(queries, c["candidates"], k, c["target"], c["alpha"])
    st_on, f = ivf.stats, ivf.filter_stats()
    assert chosen_on == chosen_off and sweep_on == sweep_off
    for name in STAT_FIELDS:
        assert getattr(st_on, name) == getattr(st_off, name), name
    assert f.queries_filtered == len(queries) * len(sweep_on) and f.rows_filtered == st_on.rows_scored and f.rows_rescored < f.rows_filtered
    # an unknown mode is refused and nothing changes
    before = (ivf.list_filter, ivf.stats, ivf.filter_stats())
    for mode in (2, 7, 0xFFFFFFFF):
        assert L.fsgpu_ivf_set_list_filter(ivf._h, mode) == fa._lib.ERR_INVALID_CONFIG
    assert (ivf.list_filter, ivf.stats, ivf.filter_stats()) == before
    fresh = idx.build_ivf(4, iters=0)
    assert L.fsgpu_ivf_set_list_filter(fresh._h, 3) == fa._lib.ERR_INVALID_CONFIG
    assert not fresh.list_filter and fresh.filter_stats().copy_bytes == 0   # nothing was built
    # off restores today's launches: a coarse search and one gather scan
    ivf.search_batched(queries, k, 4)
    assert ivf.stats.launches == 4   # ... the score and the selection besides
    ivf.set_list_filter(False)
    assert not ivf.list_filter
    ivf.search_batched(queries, k, 4)
    assert ivf.stats.launches == 2 and ivf.filter_stats().mode == 0
    # a generation change: the handle is refused as it is today, by the mode switch too
    ivf.set_list_filter(True)
    live2 = np.ones(slab.shape[0], dtype=bool)
    live2[::5] = False
    idx.set_live(live2)
    assert idx.vacuum().tombstones_removed == int((~live2).sum())
    with pytest.raises(fa.InvalidConfig):
        ivf.search_batched(queries, k, 4)
    with pytest.raises(fa.InvalidConfig):
        ivf.set_list_filter(False)
    assert "stale" in fa._lib.last_error()

"""CPU checks for fsgpu_search_hits_batched: tests/search_hits_ref.py — the restatement the GPU tests compare the WAL
kernel with — is pinned against the oracle (fso_dot_f32_f32, fso_fsvi_append / _soft_delete / _search), the reference's own WAL
shadowing case and the tie rule; the new C entry points exist, are bound, and answer with a status on a host without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import search_hits_ref as R  # noqa: E402

F32 = np.float32
NEW = ["fsgpu_search_hits_batched", "fsgpu_search_hits_batched_device_queries", "fsgpu_search_hits_two_pass_batched"]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


@pytest.mark.parametrize("hreduce", [R.HREDUCE_SSE2, R.HREDUCE_AVX, R.HREDUCE_SEQ])
def test_dot_restatement_equals_the_oracle_bit_for_bit(oracle, hreduce):
    rng = np.random.default_rng(11)
    for dim in (1, 4, 7, 8, 31, 32, 33, 36, 40, 63, 64, 72, 100, 256, 257, 384):
        wal = rng.standard_normal((9, dim)).astype(F32)
        q = rng.standard_normal(dim).astype(F32)
        got = R.wal_scores(wal, q, hreduce)
        want = np.array([oracle.dot_f32_f32(wal[w], q, hreduce) for w in range(9)], F32)
        assert np.array_equal(bits(got), bits(want)), dim
    # an overflowing score: one huge product, everything else zero -> +inf in both
    wal = np.zeros((2, 40), F32)
    wal[0, 0], wal[1, 39] = 1e19, 1e19
    q = np.zeros(40, F32)
    q[0], q[39] = 3e38, 3e38
    got = R.wal_scores(wal, q, hreduce)
    assert np.all(np.isposinf(got))
    assert np.array_equal(bits(got), bits([oracle.dot_f32_f32(wal[w], q, hreduce) for w in range(2)]))


def _live_of(f):
    return np.array([(f.flags(r) & 1) == 0 for r in range(f.record_count)], bool)


def _restated(oracle, f, main_ids, q, k, hreduce=0):
    """search_hits of the restatement on the oracle handle's state: main top-k by the oracle's row-level search, the rest restated."""
    live = _live_of(f)
    rows, scores = oracle.search_top_k(f.slab(), q, k, live, hreduce=hreduce) if live.any() else (np.empty(0, np.uint32), np.empty(0, F32))
    W = f.wal_record_count
    wal_ids = [f.doc_id(f.record_count + w) for w in range(W)]
    return wal_ids, live, list(zip(rows.tolist(), scores))


def test_merge_and_resolve_equal_the_oracle_on_small_files(oracle, tmp_path):
    rng = np.random.default_rng(5)
    dim, n = 40, 60
    vec = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"d{i:02d}" for i in range(n - 6)] + ["dup-a", "dup-a", "dup-a", "dup-b", "dup-b", "solo"]
    path = str(tmp_path / "small.fsvi")
    assert oracle.fsvi_write(path, list(zip(ids, vec)), "emb", "r1", 1, 1) == 0
    f = oracle.Fsvi(path)
    main_ids = [f.doc_id(r) for r in range(n)]
    wal_vecs = {}

    def append(d, v):
        assert f.append(d, v) == 0
        wal_vecs[d] = np.asarray(v, F32)

    queries = rng.standard_normal((12, dim)).astype(F32)
    steps = [lambda: None,
             lambda: f.soft_delete("d03"),
             lambda: append("new-1", rng.standard_normal(dim)),
             lambda: append("d07", -queries[0]),                      # shadows a main row, scores low for query 0
             lambda: append("dup-a", rng.standard_normal(dim)),       # tombstones ONE of three rows, shadows all
             lambda: append("new-1", rng.standard_normal(dim)),       # supersedes the resident copy
             lambda: [append(f"new-{j}", queries[j % 12] * 3) for j in range(2, 9)],
             lambda: f.soft_delete("new-3"),                          # erases a WAL entry: indices shift
             lambda: f.soft_delete("dup-b")]
    checked = shorter = 0
    for step in steps:
        step()
        for hreduce in (0, 1, 2):
            for qi, q in enumerate(queries):
                for k in (1, 3, 10, 59, 200):
                    wal_ids, live, main_hits = _restated(oracle, f, main_ids, q, k, hreduce)
                    wal = np.stack([wal_vecs[d] for d in wal_ids]) if wal_ids else np.empty((0, dim), F32)
                    sc = R.wal_scores(wal, q, hreduce) if wal_ids else np.empty(0, F32)
                    mine = R.search_hits(main_hits, sc, live, main_ids, wal_ids, k)
                    hits, want_scores = f.search_top_k(q, k, hreduce)
                    assert [h[0] for h in hits] == [r for r, _ in mine], (qi, k)
                    assert np.array_equal(bits(want_scores), bits([s for _, s in mine]))
                    # ... and the class tables say what the strings say
                    mc, wc, sh = R.class_tables(main_ids, wal_ids)
                    by_class = R.resolve_by_class(R.merge_first_k(main_hits, sc, n, k), live, mc, wc, sh, n)
                    assert by_class == mine
                    checked += 1
                    shorter += len(mine) < min(k, int(live.sum()) + len(wal_ids))
    assert checked > 1000 and shorter > 0   # (some lists came back short: shadowing / dedup did something)


def test_class_tables():
    main_ids = ["a", "b", "b", "c", "d", "d", "d"]
    wal_ids = ["x", "b", "y", "x", "d"]
    mc, wc, sh = R.class_tables(main_ids, wal_ids)
    assert mc.tolist() == [0, 1, 1, 3, 4, 4, 4]
    assert wc.tolist() == [7, 1, 9, 7, 4]
    assert sh.tolist() == [False, True, True, False, True, True, True]


def test_the_references_wal_shadowing_case(oracle, tmp_path):
    """stale_main_entry_shadowed_by_wal: main doc-a [1, 0] (an F32 file), WAL doc-a [0, 1], query [1, 0], k = 1 -> one hit, score 0."""
    path = str(tmp_path / "stale.fsvi")
    assert oracle.fsvi_write(path, [("doc-a", np.array([1.0, 0.0], F32))], "test", "r1", 1, 0) == 0
    f = oracle.Fsvi(path)
    assert f.append("doc-a", np.array([0.0, 1.0], F32)) == 0
    q = np.array([1.0, 0.0], F32)
    hits, scores = f.search_top_k(q, 1)
    assert len(hits) == 1 and hits[0][0] == 1 and hits[0][2] == "doc-a" and abs(scores[0]) < np.finfo(F32).eps
    live = _live_of(f)
    assert not live[0]                                   # the append tombstoned the main row
    sc = R.wal_scores(np.array([[0.0, 1.0]], F32), q)
    for main_hits in ([], [(0, F32(1.0))]):              # ... and a main row that still reached the list is dropped all the same
        mine = R.search_hits(main_hits, sc, None, ["doc-a"], ["doc-a"], 1 + len(main_hits))
        assert mine == [(1, F32(0.0))]
    # k = 1 with the stale main row ahead of the WAL entry: the row takes the only slot, is dropped, nothing refills the list
    assert R.search_hits([(0, F32(1.0))], sc, None, ["doc-a"], ["doc-a"], 1) == []


def test_ties_put_the_main_row_first_then_wal_entries_by_index(oracle, tmp_path):
    """One-hot rows are exact in f16 and f32: equal scores rank the main rows (by row), then the WAL entries (by WAL index)."""
    dim = 8
    e = np.eye(dim, dtype=F32)
    rows = [("m0", e[0]), ("m1", e[0]), ("m2", e[1]), ("m3", e[0] * 0.5)]
    path = str(tmp_path / "ties.fsvi")
    assert oracle.fsvi_write(path, rows, "emb", "r1", 1, 1) == 0
    f = oracle.Fsvi(path)
    for d, v in (("w0", e[0]), ("w1", e[2]), ("w2", e[0]), ("w3", e[0] * 2)):
        assert f.append(d, v) == 0
    n = f.record_count
    main_ids = [f.doc_id(r) for r in range(n)]
    q = e[0]
    hits, scores = f.search_top_k(q, 8)
    names = [h[2] for h in hits]
    assert names[0] == "w3"                                                   # 2.0
    assert sorted(names[1:3]) == ["m0", "m1"] and [h[0] for h in hits[1:3]] == sorted(h[0] for h in hits[1:3])   # 1.0: main rows, by row
    assert names[3:5] == ["w0", "w2"]                                         # 1.0: WAL entries, by WAL index
    assert names[5] == "m3"                                                   # 0.5
    wal_ids, live, main_hits = _restated(oracle, f, main_ids, q, 8)
    wal = np.stack([e[0], e[2], e[0], e[0] * 2])
    mine = R.search_hits(main_hits, R.wal_scores(wal, q), live, main_ids, wal_ids, 8)
    assert [r for r, _ in mine] == [h[0] for h in hits] and np.array_equal(bits([s for _, s in mine]), bits(scores))


def test_non_finite_wal_scores_are_skipped(oracle, tmp_path):
    dim = 40
    rows = [(f"m{i}", np.eye(dim, dtype=F32)[i]) for i in range(4)]
    path = str(tmp_path / "inf.fsvi")
    assert oracle.fsvi_write(path, rows, "emb", "r1", 1, 1) == 0
    f = oracle.Fsvi(path)
    big = np.zeros(dim, F32)
    big[5] = 1e19                                      # finite vector, finite norm: the append accepts it
    assert f.append("big", big) == 0 and f.append("ok", np.eye(dim, dtype=F32)[5]) == 0
    q = np.zeros(dim, F32)
    q[5] = 3e38                                        # big . q overflows to +inf
    hits, _ = f.search_top_k(q, 6)
    assert "big" not in [h[2] for h in hits] and hits[0][2] == "ok"
    main_ids = [f.doc_id(r) for r in range(4)]
    wal_ids, live, main_hits = _restated(oracle, f, main_ids, q, 6)
    sc = R.wal_scores(np.stack([big, np.eye(dim, dtype=F32)[5]]), q)
    assert np.isposinf(sc[0])
    mine = R.search_hits(main_hits, sc, live, main_ids, wal_ids, 6)
    assert [r for r, _ in mine] == [h[0] for h in hits]


def test_new_entry_points_exist_and_are_bound():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build

    build()
    L = C.CDLL(_lib.LIB_PATH)
    for name in NEW + ["fsgpu_lab_index_wal_scores"]:
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES, name
    header = open(os.path.join(ROOT, "include", "fsgpu.h")).read()
    lab = open(os.path.join(ROOT, "include", "fsgpu_lab.h")).read()
    assert all(name + "(" in header for name in NEW) and "fsgpu_lab_index_wal_scores(" in lab


def test_new_entry_points_answer_with_a_status_without_a_handle():
    """No GPU is needed to be refused: a null handle is FSGPU_ERR_NULL_ARGUMENT, not a crash.  A null handle is all a host without a
    device can offer — every constructor of an index needs the GPU (fsgpu_index_create / _open_fsvi upload the slab:
    tests/test_abi_symbols.py::test_no_gpu_fails_loudly) — so the checks behind the handle (bits other than 8 / 4, a query of the
    wrong length, an index without a doc-id table, a null output) are in tests/test_gpu_search_hits_batched.py."""
    from frankensearch_amd import _lib

    L = _lib.lib()
    q = np.zeros(8, F32)
    rows, scores, counts = np.zeros(4, np.uint32), np.zeros(4, F32), np.zeros(1, np.uint32)
    fb = C.c_uint32(7)
    p = lambda a: a.ctypes.data   # noqa: E731
    assert L.fsgpu_search_hits_batched(None, p(q), 1, 8, 4, p(rows), p(scores), p(counts), C.byref(fb)) != 0
    assert L.fsgpu_search_hits_batched_device_queries(None, p(q), 1, 8, 4, p(rows), p(scores), p(counts), C.byref(fb)) != 0
    assert L.fsgpu_search_hits_two_pass_batched(None, p(q), 1, 8, 4, 3, 8, p(rows), p(scores), p(counts), C.byref(fb)) != 0
    assert L.fsgpu_lab_index_wal_scores(None, p(q), 1, p(scores)) != 0

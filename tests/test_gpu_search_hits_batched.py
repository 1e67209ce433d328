"""GPU checks of fsgpu_search_hits_batched / _device_queries / _two_pass_batched (search_hits_kernels.hip, vector_index_hits.cpp;
DESIGN 3.14).  Every whole-call assertion compares THREE answers — the batch call, the per-query fsgpu_search_hits on the same handle
and the oracle's fso_fsvi_search on the same file after the same writes (the first two share code) — in rows, score bits and counts.
The WAL kernel's arithmetic is compared bit for bit with tests/search_hits_ref.py through the lab entry point."""
import ctypes as C
import os
import shutil
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import search_hits_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
N, DIM, NQ = 40_000, 256, 300      # above the 4 * 8192-row gate of the int8 filter; 300 queries = one wide pass + a tail
_cache = {}                        # computed once, never changed


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def _check(fa, status):
    from frankensearch_amd.errors import check
    check(status)


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the 40,000 x 256 file, its queries and the three WAL states ---------------------------------------------------------------------
def _matrix_base(oracle, tmp_path_factory):
    if "base" not in _cache:
        rng = np.random.default_rng(2024)
        vec = rng.standard_normal((N, DIM)).astype(F32)
        ids = [f"doc-{i:06d}" for i in range(N)]
        target = np.arange(NQ) * 7                      # query j looks for row target[j] ...
        for t in target:                                # ... whose doc id a near copy of it carries too: duplicate ids in the main table,
            ids[t + 1] = ids[t]                         # both among the best of query j
            vec[t + 1] = vec[t] * F32(0.9)
        ids[5001] = ids[5002] = ids[5000]               # a triple that no query looks for
        queries = (vec[target] + F32(0.5) * rng.standard_normal((NQ, DIM)).astype(F32)).astype(F32)
        path = str(tmp_path_factory.mktemp("hits") / "main.fsvi")
        assert oracle.fsvi_write(path, list(zip(ids, vec)), "emb", "r1", 1, 1) == 0
        _cache["base"] = (path, ids, vec, target, queries)
    return _cache["base"]


def _wal_entries(ids, target, queries):
    """700 appends: new ids that rank first, ids of main rows that rank first with a vector that scores low (the list comes back
    short), exact copies of other entries under another id (ties), an id appended twice (the second supersedes), filler."""
    rng = np.random.default_rng(77)
    out = []
    for j in range(0, 120):
        out.append((f"new-{j:03d}", queries[j] * F32(1.0 + 0.01 * (j % 5))))
    for j in range(100, 200):
        out.append((ids[target[j]], -queries[j]))                       # shadows rows target[j] and target[j] + 1
    for j in range(0, 60):
        out.append((f"tie-{j:03d}", queries[j] * F32(1.0 + 0.01 * (j % 5))))   # same vector as new-j: equal score, later WAL index
    out.append(("new-005", queries[5] * F32(0.25)))                     # new-005 again: the resident copy is superseded
    out.append((ids[5000], queries[299]))                               # the triple: one row tombstoned, three shadowed
    while len(out) < 701:                                               # (701 appends, 700 resident entries)
        out.append((f"fill-{len(out):04d}", rng.standard_normal(DIM).astype(F32)))
    return out


def _state(fa, oracle, tmp_path_factory, name):
    """(index handle, oracle handle) in one of the states  w0: soft deletes only / w1: + one WAL entry / w700: + 700, then more deletes."""
    if name not in _cache:
        path, ids, vec, target, queries = _matrix_base(oracle, tmp_path_factory)
        idx, f = fa.VectorIndex.open(path), oracle.Fsvi(path)
        for j in range(200, 215):                                       # soft deletes BEFORE the appends: best rows of queries 200..214
            assert idx.soft_delete(ids[target[j]]) and f.soft_delete(ids[target[j]])
        if name == "w1":
            idx.append(ids[target[0]], -queries[0])
            assert f.append(ids[target[0]], -queries[0]) == 0
        if name == "w700":
            entries = _wal_entries(ids, target, queries)
            idx.append_batch(entries[:400])
            idx.append_batch(entries[400:])
            for d, v in entries:
                assert f.append(d, v) == 0
            for d in ("new-007", ids[target[220]], "tie-003"):          # soft deletes AFTER: WAL entries erased (indices shift), a main id
                assert idx.soft_delete(d) and f.soft_delete(d)
        want_w = {"w0": 0, "w1": 1, "w700": 698}[name]
        assert idx.wal_record_count() == want_w == f.wal_record_count
        _cache[name] = (idx, f)
    return _cache[name]


def _oracle_answers(f, queries, k, hreduce=0):
    out = []
    for q in queries:
        hits, scores = f.search_top_k(q, k, hreduce)
        out.append(([h[0] for h in hits], scores))
    return out


def _per_query(fa, idx, queries, k):
    L = fa._lib.lib()
    out = []
    rows, scores, n = np.empty(max(k, 1), np.uint32), np.empty(max(k, 1), F32), C.c_uint32()
    for q in queries:
        q = np.ascontiguousarray(q, F32)
        _check(fa, L.fsgpu_search_hits(idx._h, q.ctypes.data, q.size, k, rows.ctypes.data, scores.ctypes.data, C.byref(n)))
        out.append((rows[:n.value].tolist(), scores[:n.value].copy()))
    return out


def _assert_three_way(batch, lone, want, label):
    rows, scores, counts, _ = batch
    assert len(lone) == len(want) == rows.shape[0]
    for qi, ((lr, ls), (wr, ws)) in enumerate(zip(lone, want)):
        c = int(counts[qi])
        got_r, got_s = rows[qi, :c].tolist(), scores[qi, :c]
        assert got_r == lr == wr, (label, qi, c, len(lr), len(wr))
        assert np.array_equal(bits(got_s), bits(ls)) and np.array_equal(bits(got_s), bits(ws)), (label, qi)


@pytest.mark.parametrize("k", [1, 10, 30, 64, 256])
@pytest.mark.parametrize("state", ["w0", "w1", "w700"])
def test_whole_call_on_the_matrix_path(oracle, tmp_path_factory, state, k):
    fa = _fa()
    idx, f = _state(fa, oracle, tmp_path_factory, state)
    queries = _matrix_base(oracle, tmp_path_factory)[4]
    want = _oracle_answers(f, queries, k)
    lone = _per_query(fa, idx, queries, k)
    short = 0
    for nq in (1, 130, NQ):
        batch = idx.search_hits_batched_raw(queries[:nq], k)
        print(f"state {state} k {k} nq {nq}: fallbacks {batch[3]}")
        _assert_three_way(batch, lone[:nq], want[:nq], (state, k, nq))
        if k <= 64:
            assert batch[3] == 0, (state, k, nq, batch[3])     # a batch that fell back would equal the per-query answer trivially
        short += int(np.sum(batch[2] < k))
    if state != "w0" and k > 1:
        assert short > 0        # shadowing / dedup cut some lists short, and nothing refilled them
    if state == "w700" and k >= 10:
        # ties: new-j and tie-j carry one vector, so they score alike and rank by WAL index
        rows, _, counts, _ = idx.search_hits_batched_raw(queries[:60], k)
        seen = 0
        for qi in range(60):
            names = [idx.doc_id_at(int(r)) for r in rows[qi, :counts[qi]]]
            if qi != 5 and f"new-{qi:03d}" in names and f"tie-{qi:03d}" in names:   # (new-005 was superseded by another vector)
                assert names.index(f"tie-{qi:03d}") == names.index(f"new-{qi:03d}") + 1
                seen += 1
        assert seen >= 40


def test_python_wrappers_resolve_doc_ids(oracle, tmp_path_factory):
    fa = _fa()
    idx, f = _state(fa, oracle, tmp_path_factory, "w700")
    queries = _matrix_base(oracle, tmp_path_factory)[4][:5]
    lists = idx.search_hits_batched(queries, 10)
    for qi, hits in enumerate(lists):
        one = idx.search_top_k(queries[qi], 10)
        assert [(h.index, h.doc_id) for h in hits] == [(h.index, h.doc_id) for h in one]
        assert np.array_equal(bits([h.score for h in hits]), bits([h.score for h in one]))


def test_device_queries_form_gives_the_same_bits(oracle, tmp_path_factory):
    import torch
    fa = _fa()
    idx, f = _state(fa, oracle, tmp_path_factory, "w700")
    queries = _matrix_base(oracle, tmp_path_factory)[4][:130]
    host = idx.search_hits_batched_raw(queries, 30)
    qd = torch.from_numpy(queries).to("cuda:0").contiguous()
    torch.cuda.synchronize()
    dev = idx.search_hits_batched_raw(None, 30, queries_ptr=qd.data_ptr(), nq=130)
    assert np.array_equal(host[2], dev[2]) and host[3] == dev[3] == 0
    for qi in range(130):
        c = int(host[2][qi])
        assert np.array_equal(host[0][qi, :c], dev[0][qi, :c]) and np.array_equal(bits(host[1][qi, :c]), bits(dev[1][qi, :c]))
    _assert_three_way(dev, _per_query(fa, idx, queries, 30), _oracle_answers(f, queries, 30), "device queries")


@pytest.mark.parametrize("bits_", [8, 4])
def test_two_pass_form(oracle, tmp_path_factory, bits_):
    fa = _fa()
    queries = _matrix_base(oracle, tmp_path_factory)[4][:130]
    k, mult = 10, 3
    lone_fn = lambda idx, q: (idx.search_top_k_int8_two_pass if bits_ == 8 else idx.search_top_k_4bit_two_pass)(q, k, mult)   # noqa: E731
    # no WAL: the row-level batched two-pass, then the dedup on the device — no fallbacks
    idx, f = _state(fa, oracle, tmp_path_factory, "w0")
    rows, scores, counts, fb = idx.search_hits_batched_raw(queries, k, two_pass=(mult, bits_))
    print(f"two-pass bits {bits_}: fallbacks {fb}")
    assert fb == 0
    deduped = 0
    for qi in range(130):
        one = lone_fn(idx, queries[qi])
        c = int(counts[qi])
        assert rows[qi, :c].tolist() == [h.index for h in one], qi
        assert np.array_equal(bits(scores[qi, :c]), bits([h.score for h in one]))
        deduped += c < k
    assert deduped > 0      # (query j's two best rows share a doc id)
    # one WAL entry: the exact path, like the reference (search.rs:579-585)
    idx, f = _state(fa, oracle, tmp_path_factory, "w1")
    batch = idx.search_hits_batched_raw(queries, k, two_pass=(mult, bits_))
    lone = [([h.index for h in hs], np.array([h.score for h in hs], F32)) for hs in (lone_fn(idx, q) for q in queries)]
    _assert_three_way(batch, lone, _oracle_answers(f, queries, k), ("two-pass", bits_))
    assert batch[3] == 0


def test_staleness_every_write_rebuilds_the_device_tables(oracle, tmp_path_factory, tmp_path):
    fa = _fa()
    base, ids, vec, target, queries = _matrix_base(oracle, tmp_path_factory)
    path = str(tmp_path / "stale.fsvi")
    shutil.copy(base, path)
    idx, f = fa.VectorIndex.open(path), oracle.Fsvi(path)
    queries, k = queries[:130], 10

    def check(label):
        batch = idx.search_hits_batched_raw(queries, k)
        _assert_three_way(batch, _per_query(fa, idx, queries, k), _oracle_answers(f, queries, k), label)
        assert batch[3] == 0
        return batch

    check("fresh")
    entries = [(f"new-{j}", queries[j]) for j in range(40)] + [(ids[target[j]], -queries[j]) for j in range(40, 80)]
    idx.append_batch(entries)
    for d, v in entries:
        assert f.append(d, v) == 0
    b1 = check("after append_batch")
    assert any(idx.doc_id_at(int(b1[0][j, 0])) == f"new-{j}" for j in range(40))
    assert idx.soft_delete("new-3") and f.soft_delete("new-3")          # a WAL id: the entries behind it move down
    check("after soft_delete of a WAL id")
    idx.compact(path)                                                   # the WAL folds into the slab; the new image is on disk
    assert idx.wal_record_count() == 0
    f = oracle.Fsvi(path)
    check("after compact")
    idx.append("late", queries[7] * F32(2))
    assert idx.soft_delete(ids[target[90]])                             # two tombstoned rows for the vacuum to drop
    idx.vacuum(path)                                                    # tombstoned rows leave the slab: rows renumber; the WAL stays
    f = oracle.Fsvi(path)
    assert f.append("late", queries[7] * F32(2)) == 0
    b = check("after vacuum")
    assert idx.doc_id_at(int(b[0][7, 0])) == "late"
    idx.close()


# ---- the general path: small files, an F32 slab, k beyond the device path -------------------------------------------------------------
@pytest.mark.parametrize("dim,quant", [(384, 1), (40, 0)])
def test_whole_call_on_the_general_path(oracle, tmp_path, dim, quant):
    fa = _fa()
    rng = np.random.default_rng(dim)
    n, nq = 3000, 70
    vec = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"g-{i:05d}" for i in range(n)]
    for t in range(0, 700, 10):
        ids[t + 1] = ids[t]
        vec[t + 1] = vec[t] * F32(0.9)
    queries = (vec[np.arange(nq) * 10] + F32(0.5) * rng.standard_normal((nq, dim)).astype(F32)).astype(F32)
    if quant == 0:
        queries[3] = 0
        queries[3, 5] = 3e38                                           # with the entry below: a WAL score that overflows to +inf
    path = str(tmp_path / "general.fsvi")
    assert oracle.fsvi_write(path, list(zip(ids, vec)), "emb", "r1", 1, quant) == 0
    idx, f = fa.VectorIndex.open(path), oracle.Fsvi(path)
    big = np.zeros(dim, F32)
    big[5] = 1e19                                                      # finite values, finite norm: wal_append accepts it
    entries = [("big", big)] + [(f"new-{j}", queries[j]) for j in range(4, 30)] + [(ids[j * 10], -queries[j]) for j in range(30, 55)]
    idx.append_batch(entries)
    for d, v in entries:
        assert f.append(d, v) == 0
    assert idx.soft_delete(ids[600]) and f.soft_delete(ids[600])
    W = idx.wal_record_count()
    for k in (10, 64, 256, n + W + 5):                                 # the last: collect-all, beyond the device path (per query, counted)
        batch = idx.search_hits_batched_raw(queries, k)
        print(f"general dim {dim} quant {quant} k {k}: fallbacks {batch[3]}")
        _assert_three_way(batch, _per_query(fa, idx, queries, k), _oracle_answers(f, queries, k), (dim, quant, k))
        if k > 256:
            assert batch[3] == nq
        if quant == 0:
            names = [idx.doc_id_at(int(r)) for r in batch[0][3, :batch[2][3]]]
            assert "big" not in names                                  # the non-finite score was skipped
    idx.close()


def test_a_tiny_index_on_the_device_path_and_argument_checks(oracle, tmp_path):
    """100 rows + 20 WAL entries, k = 256 >= rows + W on the DEVICE path: the main list is short, kw = W < k, every live document comes
    back once.  Then the arguments the new calls refuse with a status."""
    fa = _fa()
    L = fa._lib.lib()
    rng = np.random.default_rng(31)
    n, dim, nq = 100, 256, 9
    vec = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"t-{i:03d}" for i in range(n)]
    ids[11] = ids[10]
    queries = rng.standard_normal((nq, dim)).astype(F32)
    path = str(tmp_path / "tiny.fsvi")
    assert oracle.fsvi_write(path, list(zip(ids, vec)), "emb", "r1", 1, 1) == 0
    idx, f = fa.VectorIndex.open(path), oracle.Fsvi(path)
    entries = [(ids[i], rng.standard_normal(dim).astype(F32)) for i in (3, 10, 50)] + \
              [(f"new-{j}", rng.standard_normal(dim).astype(F32)) for j in range(17)]
    idx.append_batch(entries)
    for d, v in entries:
        assert f.append(d, v) == 0
    assert idx.soft_delete(ids[70]) and f.soft_delete(ids[70])
    for k in (256, 130, 20, 7):
        batch = idx.search_hits_batched_raw(queries, k)
        _assert_three_way(batch, _per_query(fa, idx, queries, k), _oracle_answers(f, queries, k), ("tiny", k))
    assert int(batch[2][0]) == 7
    full = idx.search_hits_batched_raw(queries, 256)
    assert np.all(full[2] == 115)      # 99 distinct main ids - the deleted one + 17 new ones: every live document once
    p = lambda a: a.ctypes.data   # noqa: E731
    rows, scores, counts, fb = np.zeros((nq, 4), np.uint32), np.zeros((nq, 4), F32), np.zeros(nq, np.uint32), C.c_uint32()
    args = (p(queries), nq, dim, 4)
    assert L.fsgpu_search_hits_two_pass_batched(idx._h, *args, 3, 5, p(rows), p(scores), p(counts), C.byref(fb)) == 2    # bits = 5: FSGPU_ERR_INVALID_CONFIG
    assert L.fsgpu_search_hits_batched(idx._h, p(queries), nq, dim - 1, 4, p(rows), p(scores), p(counts), C.byref(fb)) != 0   # dimension mismatch
    bare = fa.VectorIndex.from_slab(vec.astype(np.float16).view(np.uint16))
    for st in (L.fsgpu_search_hits_batched(bare._h, *args, p(rows), p(scores), p(counts), C.byref(fb)),
               L.fsgpu_search_hits_two_pass_batched(bare._h, *args, 3, 8, p(rows), p(scores), p(counts), C.byref(fb)),
               L.fsgpu_search_hits(bare._h, p(queries), dim, 4, p(rows), p(scores), C.byref(fb))):
        assert st == 2                                   # no doc-id table: FSGPU_ERR_INVALID_CONFIG, the status of fsgpu_search_hits
    assert L.fsgpu_search_hits_batched(idx._h, p(queries), nq, dim, 4, None, p(scores), p(counts), C.byref(fb)) != 0          # null output
    bare.close()
    idx.close()


# ---- the WAL kernel alone ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dim", [4, 8, 36, 40, 256, 384])
def test_wal_kernel_scores_equal_the_restatement_bit_for_bit(oracle, tmp_path, dim):
    """dims: tail only / one chunk / one group and a tail / one group and a leftover chunk / the tiers' dimensions."""
    fa = _fa()
    L = fa._lib.lib()
    rng = np.random.default_rng(900 + dim)
    path = str(tmp_path / "lab.fsvi")
    assert oracle.fsvi_write(path, [(f"m{i}", rng.standard_normal(dim).astype(F32)) for i in range(8)], "emb", "r1", 1, 1) == 0
    idx = fa.VectorIndex.open(path)
    wmax, nqmax = 2500, 257
    wal = rng.standard_normal((wmax, dim)).astype(F32)
    wal[0] = 0
    wal[0, 0] = 1e19                                                   # accepted by wal_append (finite norm) ...
    queries = rng.standard_normal((nqmax, dim)).astype(F32)
    queries[2] = 0
    queries[2, 0] = 3e38                                               # ... and overflows to +inf against this query
    per_query = [R.wal_scores_modes(wal, q) for q in queries]
    want = {h: np.stack([m[h] for m in per_query]) for h in (0, 1, 2)}     # [nq, W], once
    assert np.isposinf(want[0][2, 0])
    have = 0
    for W in (1, 63, 64, 65, 1000, 2500):
        idx.append_batch([(f"w{w:04d}", wal[w]) for w in range(have, W)])      # new ids only: the WAL grows in place
        have = W
        assert idx.wal_record_count() == W
        for h in (0, 1, 2):
            idx.set_hreduce(h)
            for nq in (1, 3, 64, 257):
                out = np.full((nq, W), np.nan, F32)
                q = np.ascontiguousarray(queries[:nq])
                _check(fa, L.fsgpu_lab_index_wal_scores(idx._h, q.ctypes.data, nq, out.ctypes.data))
                assert np.array_equal(bits(out), bits(want[h][:nq, :W])), (dim, W, h, nq)
    idx.close()


# ---- the many-queries engine ---------------------------------------------------------------------------------------------------------
def test_engine_answers_fsvi_tiers_through_the_batched_hits(oracle, tmp_path):
    fa = _fa()
    from frankensearch_amd.host import NativeTwoTierSearcher
    from frankensearch_amd.synthetic import random_bert_weights

    rng = np.random.default_rng(404)
    n, k = 40_000, 10
    ids = [f"note-{i:05d}-{'x' * (i % 4)}" for i in range(n)]
    pf, pq = str(tmp_path / "vector.fast.idx"), str(tmp_path / "vector.quality.idx")
    fa.write_fsvi(pf, list(zip(ids, rng.standard_normal((n, 256)).astype(F32))), "potion", "r1")
    fa.write_fsvi(pq, list(zip(ids, rng.standard_normal((n, 384)).astype(F32))), "minilm", "r1")
    fast, qual = fa.VectorIndex.open(pf), fa.VectorIndex.open(pq)
    m2v = fa.Model2VecEmbedder(rng.standard_normal((5000, 256)).astype(F32))
    bert = fa.NativeEmbedder(random_bert_weights(5, 3000, 384, 6, 1536))
    qual.append_batch([(ids[i], rng.standard_normal(384).astype(F32)) for i in range(0, 300, 3)] +
                      [(f"fresh-{i}", rng.standard_normal(384).astype(F32)) for i in range(50)])   # a resident WAL on the quality tier
    assert qual.wal_record_count() == 150
    nq = 60
    fq = [rng.integers(0, 5000, int(rng.integers(1, 24))).tolist() for _ in range(nq)]
    qq = [[101] + rng.integers(1000, 3000, int(rng.integers(2, 30))).tolist() + [102] for _ in range(nq)]
    lex = [[(ids[int(r)], float(30 - i)) for i, r in enumerate(rng.choice(n, 30, replace=False))] for _ in range(nq)]
    for mult in (0, 3):
        t = NativeTwoTierSearcher(fast, qual, m2v, bert, doc_id_mode=0, fast_tier_int8_multiplier=mult)
        ini, fin, rf, st = t.search_many(fq, qq, k, lex, chunk=25)
        print(f"engine mult {mult}: fast fallbacks {st['fast_fallbacks']} quality fallbacks {st['quality_fallbacks']}")
        assert st["chunks"] == 3 and st["quality_fallbacks"] == 0, st
        for qi in range(nq):
            i1, f1, _ = t.search(fq[qi], qq[qi], k, lex[qi])
            assert i1 == ini[qi], (mult, qi)
        t.close()
    for h in (fast, qual, m2v, bert):
        h.close()

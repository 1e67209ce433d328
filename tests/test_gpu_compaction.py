"""GPU checks of fsgpu_index_compact / _vacuum / _wal_append_batch (compact_kernels.hip, vector_index_compact.cpp), all through the
C ABI.  The file a rewrite leaves equals, byte for byte, what the oracle's FSVI writer makes of the rows tests/compaction_ref.py
says survive; the device slab is that file's slab (every row, as bit patterns); nothing derived from the old rows answers afterwards;
offsets are 64-bit; append_batch is all-or-nothing; sharded, table-less and busy handles are refused unchanged."""
import os
import shutil
import sys
import threading

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compaction_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
N = 3001            # rows of the byte-level cases: with 1,000 rows per launch (lab setter) the runs cross launch and wave boundaries
LAUNCH_ROWS = 1000
PATTERNS = ["none", "first", "last", "alternating", "block1000", "all"]
SHAPES = [(4, "f16"), (43, "f16"), (100, "f16"), (384, "f16"), (43, "f32"), (384, "f32")]
_base = {}          # (dim, quant, gen) -> (rows, path of the oracle-written file): computed once, never changed


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _qcode(quant):
    return 1 if quant == "f16" else 0


def _base_case(oracle, tmp_path_factory, dim, quant, gen=1):
    key = (dim, quant, gen)
    if key not in _base:
        rng = np.random.default_rng(1000 + dim)
        vec = rng.standard_normal((N, dim)).astype(F32)
        ids = [f"doc-{i:05d}" for i in range(N - 2)] + ["twin", "twin"]   # one doc id twice live in the file
        rows = list(zip(ids, vec))
        path = str(tmp_path_factory.mktemp("compaction") / f"base-{dim}-{quant}-{gen}.fsvi")
        assert oracle.fsvi_write(path, rows, "emb", "r1", gen, _qcode(quant)) == 0
        m = R.Model(rows, dim, quant, gen, "emb", "r1")
        assert open(path, "rb").read() == m.image()
        _base[key] = (rows, path)
    return _base[key]


def _live_mask(pattern):
    live = np.ones(N, bool)
    if pattern == "first":
        live[0] = False
    elif pattern == "last":
        live[-1] = False
    elif pattern == "alternating":
        live[1::2] = False
    elif pattern == "block1000":
        live[777:1777] = False
    elif pattern == "all":
        live[:] = False
    return live


def _id_beyond(m, before):
    """A doc id that sorts before the first / after the last main row."""
    edge = R.sort_key(m.main[0][0]) if before else R.sort_key(m.main[-1][0])
    i = 0
    while True:
        d = f"edge-{i}"
        k = R.sort_key(d)
        if (k < edge) if before else (k > edge):
            return d
        i += 1


def _open_case(fa, oracle, tmp_path_factory, tmp_path, dim, quant, pattern, gen=1):
    """A fresh handle over a private copy of the base file + the model, after the same tombstones and WAL writes on both."""
    rows, base = _base_case(oracle, tmp_path_factory, dim, quant, gen)
    path = str(tmp_path / f"{dim}-{quant}-{pattern}-{len(os.listdir(tmp_path))}.fsvi")
    shutil.copy(base, path)
    idx = fa.VectorIndex.open(path)
    fa._lib.lib().fsgpu_lab_index_set_compact_launch_rows(idx._h, LAUNCH_ROWS)
    m = R.Model(rows, dim, quant, gen, "emb", "r1")
    if pattern != "none":
        live = _live_mask(pattern)
        idx.set_live(live)
        m.set_live(live)
    rng = np.random.default_rng(7)
    v = lambda: rng.standard_normal(dim).astype(F32)   # noqa: E731
    between = "between-rows"
    writes = [(_id_beyond(m, True), v()), (_id_beyond(m, False), v()), (between, v()),
              (m.main[100][0], v()),          # supersedes a main row (live unless the pattern tombstoned it)
              ("twin", v()),                  # a doc id present twice live in the file
              ("gone", v()), ("again", v()), ("again", v())]
    for d, x in writes:
        idx.append(d, x)
        m.append(d, x)
    assert idx.soft_delete("gone") and m.soft_delete("gone")
    assert idx.wal_record_count() == len(m.wal) and idx.tombstone_count() == m.tombstone_count()
    return idx, m, path


def _expected_file(oracle, tmp_path, m):
    want = m.image()
    if m.main:   # (the oracle's writer refuses an empty row list: the restated image alone then, pinned against it on the CPU)
        p = str(tmp_path / "want.fsvi")
        assert oracle.fsvi_write(p, m.writer_rows(), m.embedder_id, m.revision, m.gen, _qcode(m.quant)) == 0
        assert open(p, "rb").read() == want
    return want


def _check_handle(idx, m):
    n = len(m.main)
    assert idx.record_count() == n and idx.tombstone_count() == 0 and idx.live_count() == n
    assert idx.wal_record_count() == len(m.wal)
    for i, (d, raw) in enumerate(m.rows()):
        assert idx.doc_id_at(i) == d, i
        got = idx.vector_at(i)
        assert np.array_equal(bits(got), bits(R.widen_row(raw, m.quant))), (i, d)
    for w, (d, _) in enumerate(m.wal):
        assert idx.doc_id_at(n + w) == d


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dim,quant", SHAPES)
def test_compact_file_bytes_and_device_slab(oracle, tmp_path_factory, tmp_path, dim, quant, pattern):
    fa = _fa()
    for with_file in (True, False):
        idx, m, path = _open_case(fa, oracle, tmp_path_factory, tmp_path, dim, quant, pattern)
        g0 = idx.generation()
        st = idx.compact(path if with_file else None)
        want = m.compact()
        assert (st.main_records_before, st.wal_records, st.total_records_after) == \
            (want["main_records_before"], want["wal_records"], want["total_records_after"])
        assert idx.generation() == g0 + 1 and idx.compaction_gen() == m.gen == 2
        _check_handle(idx, m)
        if with_file:
            assert open(path, "rb").read() == _expected_file(oracle, tmp_path, m)
            assert not os.path.exists(path + ".tmp")
            again = fa.VectorIndex.open(path)
            _check_handle(again, m)
            again.close()
        idx.close()


@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dim,quant", SHAPES)
def test_vacuum_file_bytes_and_device_slab(oracle, tmp_path_factory, tmp_path, dim, quant, pattern):
    fa = _fa()
    for with_file in (True, False):
        idx, m, path = _open_case(fa, oracle, tmp_path_factory, tmp_path, dim, quant, pattern)
        g0 = idx.generation()
        st = idx.vacuum(path if with_file else None)
        want = m.vacuum()
        assert (st.records_before, st.records_after, st.tombstones_removed, st.bytes_reclaimed) == \
            (want["records_before"], want["records_after"], want["tombstones_removed"], want["bytes_reclaimed"])
        assert want["tombstones_removed"] >= 1 and idx.generation() == g0 + 1   # (the WAL writes tombstoned a row in every pattern)
        assert idx.compaction_gen() == m.gen == 1 and idx.wal_record_count() == len(m.wal) == 6
        _check_handle(idx, m)
        if with_file:
            assert open(path, "rb").read() == _expected_file(oracle, tmp_path, m)
        idx.close()


def test_generation_255_wraps_to_1(oracle, tmp_path_factory, tmp_path):
    fa = _fa()
    idx, m, path = _open_case(fa, oracle, tmp_path_factory, tmp_path, 43, "f16", "block1000", gen=255)
    assert idx.compaction_gen() == 255
    idx.compact(path)
    m.compact()
    assert m.gen == 1 and idx.compaction_gen() == 1
    assert open(path, "rb").read() == _expected_file(oracle, tmp_path, m)
    idx.close()


def test_nan_payloads_and_negative_zero_come_through_as_a_raw_copy(oracle, tmp_path_factory, tmp_path):
    """Main rows are copied, not decoded and re-encoded: signalling and quiet NaN payloads and -0.0 keep their f16 bits."""
    fa = _fa()
    dim = 100
    rows, base = _base_case(oracle, tmp_path_factory, dim, "f16")
    m = R.Model(rows, dim, "f16", 1, "emb", "r1")
    odd = np.frombuffer(m.main[1500][1], dtype="<u2").copy()
    odd[:6] = [0x7E01, 0xFE55, 0x7C01, 0xFC7F, 0x8000, 0x0001]   # quiet / signalling NaNs with payloads, -0.0, the least subnormal
    m.main[1500][1] = odd.tobytes()
    for with_file in (True, False):
        path = str(tmp_path / f"odd-{int(with_file)}.fsvi")
        open(path, "wb").write(m.image())   # (the header CRC does not cover the slab)
        idx = fa.VectorIndex.open(path)
        fa._lib.lib().fsgpu_lab_index_set_compact_launch_rows(idx._h, LAUNCH_ROWS)
        mm = R.Model(rows, dim, "f16", 1, "emb", "r1")
        mm.main[1500][1] = odd.tobytes()
        before = bits(idx.vector_at(1500)).copy()   # the library's own widening of these bits
        live = np.ones(N, bool)
        live[10:1400:3] = False
        live[1501] = False
        idx.set_live(live)
        mm.set_live(live)
        x = np.arange(1, dim + 1, dtype=F32)
        idx.append("fresh", x)
        mm.append("fresh", x)
        idx.compact(path if with_file else None)
        mm.compact()
        at = [i for i, (d, _) in enumerate(mm.rows()) if d == m.main[1500][0]][0]
        assert mm.rows()[at][1] == odd.tobytes() and np.array_equal(bits(idx.vector_at(at)), before)
        for i in (0, at - 1, at + 1, len(mm.main) - 1):
            assert np.array_equal(bits(idx.vector_at(i)), bits(R.widen_row(mm.rows()[i][1], "f16")))
        if with_file:
            assert open(path, "rb").read() == mm.image()   # the file's slab holds the odd row's bytes as they were
        idx.close()


def _unit_rows(rng, n, dim):
    v = rng.standard_normal((n, dim)).astype(F32)
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _same(a, b):
    return all(np.array_equal(np.asarray(x).view(np.uint32) if np.asarray(x).dtype == F32 else np.asarray(x), np.asarray(y).view(np.uint32)
                              if np.asarray(y).dtype == F32 else np.asarray(y)) for x, y in zip(a, b))


@pytest.mark.parametrize("n", [20_000, 40_000])   # 40,000: the smallest round size at which the int8 filter's copies exist (>= 32,768 rows)
def test_nothing_stale_answers_after_a_compaction(oracle, tmp_path, n):
    fa = _fa()
    dim, k = 384, 10
    rng = np.random.default_rng(3)
    vec = _unit_rows(rng, n, dim)
    ids = [f"doc-{i:06d}" for i in range(n)]
    rows = list(zip(ids, vec))
    path = str(tmp_path / "big.fsvi")
    assert oracle.fsvi_write(path, rows, "emb", "r1", 4, 1) == 0
    m = R.Model(rows, dim, "f16", 4, "emb", "r1")
    queries = _unit_rows(rng, 64, dim) + 0.5 * vec[rng.integers(0, n, 64)]
    idx = fa.VectorIndex.open(path)
    # everything the library derives from the rows, built BEFORE the compaction
    idx.set_int8_latency(True, build_now=True)
    idx.set_filter_rotation(2)
    for f in (2, 1):
        idx.set_batched_filter(f)
        idx.search_batched(queries, k)
    idx.set_batched_filter(0)
    idx.search_top_k_4bit_two_pass(queries[0], k)
    idx.search_top_k_int8_two_pass(queries[0], k)
    idx.search_int8_two_pass_batched(queries, k)
    idx.search_4bit_two_pass_batched(queries, k)
    idx.mrl_search(queries[0], k, search_dims=64)
    threads = [threading.Thread(target=lambda q=q: idx.search_batch(q, k)) for q in queries[:2] for _ in range(4)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    stale_filter = idx.resident_filter(rng.random(n) > 0.5)
    idx.search_batch(queries[:2], k, allow=stale_filter)
    # 2,000 tombstones and 500 WAL entries, a fifth of them new versions of main rows
    live = np.ones(n, bool)
    live[rng.choice(n, 2000, replace=False)] = False
    idx.set_live(live)
    m.set_live(live)
    entries = [(ids[int(i)] if j % 5 == 0 else f"new-{j:04d}", _unit_rows(rng, 1, dim)[0]) for j, i in enumerate(rng.integers(0, n, 500))]
    idx.append_batch(entries)
    m.append_batch(entries)
    assert idx.wal_record_count() == len(m.wal)
    g0 = idx.generation()
    st = idx.compact()
    want = m.compact()
    assert st.total_records_after == want["total_records_after"] == idx.record_count() and idx.generation() == g0 + 1
    fresh_path = str(tmp_path / "fresh.fsvi")
    assert oracle.fsvi_write(fresh_path, m.writer_rows(), "emb", "r1", m.gen, 1) == 0
    fresh = fa.VectorIndex.open(fresh_path)
    for f in (2, 1):
        idx.set_batched_filter(f)
        fresh.set_batched_filter(f)
        assert _same(idx.search_batched(queries, k)[:3], fresh.search_batched(queries, k)[:3]), f
    idx.set_batched_filter(0)
    fresh.set_batched_filter(0)
    assert _same(idx.search_batch(queries, k, exact=True), fresh.search_batch(queries, k, exact=True))
    assert _same(idx.search_batch(queries, k), fresh.search_batch(queries, k))
    assert _same(idx.search_int8_two_pass_batched(queries, k)[:3], fresh.search_int8_two_pass_batched(queries, k)[:3])
    assert _same(idx.search_4bit_two_pass_batched(queries, k)[:3], fresh.search_4bit_two_pass_batched(queries, k)[:3])
    for q in queries:
        assert idx.search_top_k_int8_two_pass(q, k) == fresh.search_top_k_int8_two_pass(q, k)
        assert idx.search_top_k_4bit_two_pass(q, k) == fresh.search_top_k_4bit_two_pass(q, k)
        assert idx.mrl_search(q, k, search_dims=64) == fresh.mrl_search(q, k, search_dims=64)
        assert idx.search_top_k(q, k) == fresh.search_top_k(q, k)
    with pytest.raises(fa.InvalidConfig):
        idx.search_batch(queries[:2], k, allow=stale_filter)
    with pytest.raises(fa.InvalidConfig):
        idx.search_batched(queries, k, allow=stale_filter)
    st2 = idx.compact()
    assert (st2.main_records_before, st2.wal_records, st2.total_records_after) == (idx.record_count(), 0, idx.record_count())
    assert idx.generation() == g0 + 1
    stale_filter.close()
    fresh.close()
    idx.close()


@pytest.mark.parametrize("drop", [0.01, 0.001])   # 0.001: the DESTINATION crosses 2^32 bytes as well (2,797,200 x 1,536 > 2^32)
def test_offsets_are_64_bit(drop):
    import torch
    fa = _fa()
    n, dim = 2_800_000, 768   # the smallest round row count with n * dim * 2 > 2^32
    row_bytes = dim * 2
    assert n * row_bytes > 2 ** 32 > (n - 100_000) * row_bytes
    dev = torch.device("cuda", 0)
    gen = torch.Generator(device=dev)
    gen.manual_seed(17)
    slab = torch.empty((n, dim), dtype=torch.float16, device=dev)
    for r0 in range(0, n, 400_000):
        slab[r0:r0 + 400_000].normal_(generator=gen)
    rng = np.random.default_rng(23)
    live = rng.random(n) >= drop
    live[0] = live[-1] = True
    live_idx = np.flatnonzero(live)
    bm = torch.from_numpy(fa.pack_bitmap(live).view(np.int64)).to(dev)
    idx = fa.VectorIndex.from_device_slab(slab.data_ptr(), n, dim, live_ptr=bm.data_ptr(), keepalive=(slab, bm))
    assert idx.tombstone_count() == n - live_idx.size
    st = idx.vacuum()
    assert idx.record_count() == int(live.sum()) == st.records_after and st.records_before == n
    assert st.bytes_reclaimed == (n - live_idx.size) * row_bytes and idx.generation() == 1 and idx.tombstone_count() == 0
    m = live_idx.size
    sample = set(rng.integers(0, m, 4096 - 16).tolist()) | {0, m - 1}
    edge_src = 2 ** 32 // row_bytes                       # the source row the 2^32nd byte lies in, and its neighbours
    for s in (edge_src - 1, edge_src, edge_src + 1):
        j = int(np.searchsorted(live_idx, s))
        sample |= {min(max(j + d, 0), m - 1) for d in (-1, 0, 1)}
    edge_dst = 2 ** 32 // row_bytes
    if edge_dst < m:
        sample |= {edge_dst - 1, edge_dst, edge_dst + 1} & set(range(m))
        assert m * row_bytes > 2 ** 32
    sample = np.array(sorted(sample))
    want = slab[torch.from_numpy(live_idx[sample]).to(dev)].float().cpu().numpy()
    for i, w in zip(sample, want):
        assert np.array_equal(bits(idx.vector_at(int(i))), bits(w)), int(i)
    idx.close()
    del slab, bm
    torch.cuda.empty_cache()


def _hits(idx, queries, k=5):
    return [idx.search_top_k(q, k) for q in queries]


def test_append_batch(oracle, tmp_path_factory, tmp_path):
    fa = _fa()
    dim = 43
    rows, base = _base_case(oracle, tmp_path_factory, dim, "f16")
    rng = np.random.default_rng(31)
    queries = rng.standard_normal((6, dim)).astype(F32)
    a = fa.VectorIndex.open(base)
    before = _hits(a, queries)
    v = lambda: rng.standard_normal(dim).astype(F32)   # noqa: E731
    # one non-finite vector: nothing changes
    bad = v()
    bad[7] = np.inf
    with pytest.raises(fa.InvalidConfig):
        a.append_batch([("doc-00003", v()), ("oops", bad), ("late", v())])
    with pytest.raises(fa.InvalidConfig):
        a.append_batch([("doc-00003", v()), ("zero", np.zeros(dim, F32))])
    with pytest.raises(fa.DimensionMismatch):
        a.append_batch([("doc-00003", v()), ("short", np.ones(dim - 1, F32))])
    assert a.wal_record_count() == 0 and a.tombstone_count() == 0 and _hits(a, queries) == before
    # an id three times: one entry, the last vector
    last = queries[0] * 3
    a.append_batch([("rep", v()), ("other", v()), ("rep", v()), ("rep", last)])
    assert a.wal_record_count() == 2 and [a.doc_id_at(N), a.doc_id_at(N + 1)] == ["other", "rep"]
    top = a.search_top_k(queries[0], 1)[0]
    assert top.doc_id == "rep" and top.index == N + 1
    # a batch equals the same entries one by one (main rows superseded, resident entries superseded, the twin)
    entries = [(f"doc-{i:05d}", v()) for i in (5, 17, 2000)] + [("twin", v()), ("brand-new", v()), ("rep", v()), ("doc-00017", v())]
    a2 = fa.VectorIndex.open(base)
    a2.append_batch(entries)
    b2 = fa.VectorIndex.open(base)
    for d, x in entries:
        b2.append(d, x)
    assert a2.wal_record_count() == b2.wal_record_count() == 6 and a2.tombstone_count() == b2.tombstone_count() == 4
    assert _hits(a2, queries, 20) == _hits(b2, queries, 20)
    assert [a2.doc_id_at(N + w) for w in range(6)] == [b2.doc_id_at(N + w) for w in range(6)]
    for h in (a, a2, b2):
        h.close()


def test_refusals_leave_the_index_unchanged(oracle, tmp_path):
    import torch
    from frankensearch_amd.sharded import GpuShardBackend
    fa = _fa()
    rng = np.random.default_rng(41)
    n, dim = 40_000, 384
    vec = _unit_rows(rng, n, dim)
    queries = _unit_rows(rng, 130, dim)
    # no doc-id table
    plain = fa.VectorIndex.from_slab(vec.astype(np.float16))
    before = plain.search_batch(queries[:4], 5)
    with pytest.raises(fa.InvalidConfig):
        plain.compact()
    assert _same(plain.search_batch(queries[:4], 5), before) and plain.generation() == 0
    plain.close()
    # a row-sharded catalog
    path = str(tmp_path / "s.fsvi")
    assert oracle.fsvi_write(path, [(f"doc-{i:06d}", vec[i]) for i in range(n)], "emb", "r1", 1, 1) == 0
    sh = fa.NativeShardedIndex.open(path, [0])
    sh.append("w", vec[0])
    hits = sh.search_top_k(queries[0], 5)
    for call in (sh.compact, sh.vacuum):
        with pytest.raises(fa.InvalidConfig) as err:
            call()
        assert "shard" in str(err.value)
    assert sh.search_top_k(queries[0], 5) == hits and sh.wal_record_count() == 1 and sh.record_count() == n
    sh.close()
    # a begun batched search is outstanding
    idx = fa.VectorIndex.open(path)
    idx.append("w", vec[0])
    assert idx.soft_delete("doc-000007")
    hits = idx.search_top_k(queries[0], 5)
    dev = torch.device("cuda", 0)
    be = GpuShardBackend(idx, dev, batched=True)
    q = torch.from_numpy(queries).to(dev)
    out, ticket = be.scan_begin(q, 10, packed=False)
    for call in (idx.compact, idx.vacuum):
        with pytest.raises(fa.InvalidConfig) as err:
            call()
        assert "outstanding" in str(err.value)
    be.scan_end(ticket)
    torch.cuda.synchronize()
    assert idx.generation() == 0 and idx.wal_record_count() == 1 and idx.tombstone_count() == 1 and idx.record_count() == n
    assert idx.search_top_k(queries[0], 5) == hits
    st = idx.compact()   # ... and goes through once the ticket has ended
    assert st.total_records_after == n and idx.generation() == 1
    idx.close()

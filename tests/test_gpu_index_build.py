"""GPU checks of the device-resident index builder (index_build_kernels.hip, index_builder.cpp), all through the C ABI.  The contract is
an equivalence: the file a finish leaves equals, byte for byte, what fsgpu_fsvi_write_quant writes for the same records (and what
tests/index_build_ref.py restates), and the handle it returns answers as fsgpu_index_open_fsvi of that file does — doc ids, slab bits,
search rows and score bits, and the writes an opened index takes afterwards.  Host, device and encoder adds agree; every refusal
names its row and stages nothing; the verdicts at the overflow boundary and below the underflow are the restatement's, row for row;
offsets are 64-bit."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compaction_ref as CR  # noqa: E402
import index_build_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def _q(quant):
    return 1 if quant == "f16" else 0


def _build(fa, ids, v, dim, quant, chunk, path, gen=3, splits=None, **kw):
    b = fa.IndexBuilder(dim, "emb", "r1", quantization=_q(quant), compaction_gen=gen, chunk_rows=chunk, **kw)
    for lo, hi in (splits if splits is not None else R.split_adds(len(ids))):
        b.add(ids[lo:hi], v[lo:hi])
    assert b.record_count() == len(ids)
    idx = b.finish(path)
    assert b.record_count() == len(ids)
    return b, idx


def _slab_of(image, n, dim, quant):
    row_bytes = dim * (2 if quant == "f16" else 4)
    raw = np.frombuffer(image[len(image) - n * row_bytes:], dtype="<f2" if quant == "f16" else "<f4")
    return raw.reshape(n, dim).astype(F32)


def _assert_same_handle(a, b, queries, slab=None):
    """a (built) answers as b (opened) does."""
    n, dim = b.record_count(), b.dimension()
    assert (a.record_count(), a.dimension(), a.compaction_gen()) == (n, dim, b.compaction_gen())
    assert (a.wal_record_count(), a.tombstone_count(), a.generation()) == (b.wal_record_count(), b.tombstone_count(), b.generation())
    for r in range(n):
        assert a.doc_id_at(r) == b.doc_id_at(r), r
        va = bits(a.vector_at(r))
        assert np.array_equal(va, bits(b.vector_at(r))), r
        if slab is not None:
            assert np.array_equal(va, bits(slab[r])), r
    k = min(10, max(n, 1))
    ra, sa, ca = a.search_batch(queries, k, exact=True)
    rb, sb, cb = b.search_batch(queries, k, exact=True)
    assert np.array_equal(ca, cb) and np.array_equal(ra, rb) and np.array_equal(bits(sa), bits(sb))
    for q in queries:
        ha, hb = a.search_top_k(q, k), b.search_top_k(q, k)
        assert [(h.index, h.doc_id) for h in ha] == [(h.index, h.doc_id) for h in hb]
        assert np.array_equal(bits([h.score for h in ha]), bits([h.score for h in hb]))


@pytest.mark.parametrize("case", list(enumerate(R.cases())), ids=lambda c: "%d-dim%d-n%d-chunk%d-%s" % ((c[0],) + c[1]))
def test_file_bytes_and_handle(tmp_path, case):
    fa = _fa()
    seed, (dim, n, chunk, quant) = case
    ids, v = R.fixture(dim, n, seed)
    built_path, written_path = str(tmp_path / "built.fsvi"), str(tmp_path / "written.fsvi")
    b, idx = _build(fa, ids, v, dim, quant, chunk, built_path)
    if n:
        fa.write_fsvi(written_path, list(zip(ids, v)), "emb", "r1", compaction_gen=3, quantization=_q(quant))
    else:   # (the Python wrapper takes the dimension from the first row: the C entry point directly)
        assert fa._lib.lib().fsgpu_fsvi_write_quant(written_path.encode(), b"emb", b"r1", dim, 0, None, None, None, 3, 0, _q(quant)) == 0
    image = open(built_path, "rb").read()
    assert image == open(written_path, "rb").read()
    ref = R.Builder(dim, quant, "emb", "r1", 3, chunk_rows=chunk or 65536)
    for lo, hi in R.split_adds(n):
        ref.add(ids[lo:hi], v[lo:hi])
    assert image == ref.finish()
    assert not os.path.exists(built_path + ".tmp")
    st = b.last_stats
    chunk_rows = chunk or 65536
    assert st.rows == n and st.chunks == (n + chunk_rows - 1) // chunk_rows and st.permute_launches == (1 if n else 0)
    assert st.ingest_launches == len(R.split_adds(n))
    assert st.peak_device_bytes >= st.chunks * chunk_rows * dim * (2 if quant == "f16" else 4) + n * dim * (2 if quant == "f16" else 4) + n * 4
    opened = fa.VectorIndex.open(written_path)
    queries = np.random.default_rng(seed + 500).standard_normal((3, dim)).astype(F32)
    _assert_same_handle(idx, opened, queries, _slab_of(image, n, dim, quant))
    idx.close()
    opened.close()


def test_batched_search_and_no_path(tmp_path):
    """40,000 rows: the smallest size at which the int8 filter's copies exist; and path=None gives the same handle, touching no file."""
    fa = _fa()
    n, dim = 40000, 384
    rng = np.random.default_rng(77)
    v = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"doc-{i}" for i in range(n)]
    ids[17] = ids[30000]
    p = str(tmp_path / "a.fsvi")
    _, idx = _build(fa, ids, v, dim, "f16", 0, p, splits=[(0, 9000), (9000, n)])
    before = sorted(os.listdir(tmp_path))
    _, idx_np = _build(fa, ids, v, dim, "f16", 4097, None, splits=[(0, 1), (1, n)])
    assert sorted(os.listdir(tmp_path)) == before
    fa.write_fsvi(str(tmp_path / "w.fsvi"), list(zip(ids, v)), "emb", "r1", compaction_gen=3)
    assert open(p, "rb").read() == open(str(tmp_path / "w.fsvi"), "rb").read()
    opened = fa.VectorIndex.open(str(tmp_path / "w.fsvi"))
    queries = rng.standard_normal((70, dim)).astype(F32)
    want = opened.search_batched(queries, 10)
    want_hits = opened.search_hits_batched_raw(queries, 10)
    for h in (idx, idx_np):
        got = h.search_batched(queries, 10)
        assert np.array_equal(got[0], want[0]) and np.array_equal(bits(got[1]), bits(want[1])) and np.array_equal(got[2], want[2])
        got_hits = h.search_hits_batched_raw(queries, 10)
        assert np.array_equal(got_hits[0], want_hits[0]) and np.array_equal(bits(got_hits[1]), bits(want_hits[1]))
        assert np.array_equal(got_hits[2], want_hits[2])
        assert h.batched_filter_stats()["int8_active"] == opened.batched_filter_stats()["int8_active"]
        for r in (0, 1, 17, 20000, n - 1):
            assert h.doc_id_at(r) == opened.doc_id_at(r) and np.array_equal(bits(h.vector_at(r)), bits(opened.vector_at(r)))
    for h in (idx, idx_np, opened):
        h.close()


def _tokens(rng, n, vocab, lo=3, hi=30):
    return [rng.integers(1, vocab, size=int(rng.integers(lo, hi))).tolist() for _ in range(n)]


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_routes_agree(tmp_path, quant):
    """Host, device and encoder adds of the same vectors give the same bytes; add_bert equals add of fsgpu_bert_embed's output."""
    import torch
    from oracle import bert_oracle
    fa = _fa()
    rng = np.random.default_rng(5)
    dev = torch.device("cuda", 0)
    # --- Model2Vec: synthetic table
    table = rng.standard_normal((1000, 256)).astype(F32)
    m2v = fa.Model2VecEmbedder(table)
    texts = _tokens(rng, 150, 1000)
    ids = [f"t-{i}" for i in range(len(texts))]
    vec = m2v.embed_batch_token_ids(texts)
    images = {}
    for route in ("host", "device", "encoder"):
        b = fa.IndexBuilder(256, "potion", "r", quantization=_q(quant), chunk_rows=37)
        for lo, hi in ((0, 1), (1, 65), (65, 150)):
            if route == "host":
                b.add(ids[lo:hi], vec[lo:hi])
            elif route == "device":
                t = torch.from_numpy(vec[lo:hi].copy()).to(dev)
                s = torch.cuda.Stream(device=dev)
                with torch.cuda.stream(s):
                    t2 = t * 1.0   # produced on stream s: the ingest is ordered behind it
                    b.add_device(ids[lo:hi], t2.data_ptr(), stream=s.cuda_stream)
            else:
                b.add_texts(m2v, ids[lo:hi], texts[lo:hi])
        p = str(tmp_path / f"m2v-{route}.fsvi")
        b.finish(p).close()
        images[route] = open(p, "rb").read()
    fa.write_fsvi(str(tmp_path / "m2v-w.fsvi"), list(zip(ids, vec)), "potion", "r", quantization=_q(quant))
    assert images["host"] == images["device"] == images["encoder"] == open(str(tmp_path / "m2v-w.fsvi"), "rb").read()
    # --- MiniLM-class encoder, random weights
    w = bert_oracle.random_weights(5, 500, 128, 2, 512)
    enc = fa.NativeEmbedder(w)
    btexts = [[101] + t + [102] for t in _tokens(rng, 40, 500, 2, 40)]
    bids = [f"b-{i}" for i in range(len(btexts))]
    calls = ((0, 7), (7, 40))
    host_b = fa.IndexBuilder(128, "minilm", "r", quantization=_q(quant), chunk_rows=16)
    enc_b = fa.IndexBuilder(128, "minilm", "r", quantization=_q(quant), chunk_rows=16)
    for lo, hi in calls:
        host_b.add(bids[lo:hi], enc.embed_batch_token_ids(btexts[lo:hi]))   # fsgpu_bert_embed of the same call
        enc_b.add_texts(enc, bids[lo:hi], btexts[lo:hi])
    ph, pe = str(tmp_path / "bert-h.fsvi"), str(tmp_path / "bert-e.fsvi")
    host_b.finish(ph).close()
    enc_b.finish(pe).close()
    assert open(ph, "rb").read() == open(pe, "rb").read()
    # --- an empty text embeds to zeros: refused by the norm rule, naming its row; an embedder of another dimension
    b = fa.IndexBuilder(256, "potion", "r")
    with pytest.raises(fa.InvalidConfig, match="embedding norm must be non-zero and finite") as err:
        b.add_texts(m2v, ["a", "b", "c"], [[5, 6], [], [7]])
    assert err.value.bad_row == 1 and b.record_count() == 0
    with pytest.raises(fa.DimensionMismatch):
        b.add_texts(enc, ["a"], [[101, 5, 102]])
    with pytest.raises(fa.InvalidConfig, match="embedding norm must be non-zero and finite") as err:
        fa.IndexBuilder(128, "minilm", "r").add_texts(enc, ["a", "b"], [[101, 5, 102], []])
    assert err.value.bad_row == 1


def _refused(fa, b, ids, v, rule, row, exc=None):
    n0 = b.record_count()
    with pytest.raises(exc or fa.InvalidConfig) as err:
        b.add(ids, v)
    if rule:
        assert R.RULES[rule] in str(err.value), str(err.value)
        assert err.value.bad_row == row
    assert b.record_count() == n0


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_refusals_name_the_row_and_stage_nothing(tmp_path, quant):
    fa = _fa()
    dim = 100
    rng = np.random.default_rng(3)
    good = rng.standard_normal((200, dim)).astype(F32)
    ids = [f"d{i}" for i in range(200)]
    b = fa.IndexBuilder(dim, "emb", "r1", quantization=_q(quant), chunk_rows=64)
    ref = R.Builder(dim, quant, "emb", "r1", 0, chunk_rows=64)
    b.add(ids[:70], good[:70])
    ref.add(ids[:70], good[:70])
    _refused(fa, b, ids[70:72], np.ones((2, dim + 1), F32), None, None, fa.DimensionMismatch)
    for row, col, val, rule in ((0, 0, np.nan, "nonfinite"), (129, 99, np.inf, "nonfinite"), (64, 63, -np.inf, "nonfinite"),
                                (65, 64, np.nan, "nonfinite")):
        bad = good[70:].copy()
        bad[row, col] = val
        bad[min(row + 3, 129), 5] = np.nan   # a later offender does not change the answer
        _refused(fa, b, ids[70:], bad, rule, row)
    bad = good[70:].copy()
    bad[77] = 0.0
    bad[78, 0] = np.nan
    _refused(fa, b, ids[70:], bad, "norm", 77)
    bad = good[70:].copy()
    bad[5] = 2.0e18      # 100 finite squares of 4e36: their sum passes FLT_MAX
    _refused(fa, b, ids[70:], bad, "norm", 5)
    long_ids = ids[70:]
    long_ids[9] = "y" * 65536
    _refused(fa, b, long_ids, good[70:], "doc_id_len", 9)
    bad = good[70:].copy()
    bad[9, 1] = np.nan   # the same row breaks a vector rule too: write_record judges the vector first
    _refused(fa, b, long_ids, bad, "nonfinite", 9)
    bad = good[70:].copy()
    bad[10, 1] = np.nan  # a later row's vector does not overtake an earlier row's doc id
    _refused(fa, b, long_ids, bad, "doc_id_len", 9)
    # the refused calls wrote past the count into the staging: the next add overwrites it, and finish is what it would have been
    b.add(ids[70:], good[70:])
    ref.add(ids[70:], good[70:])
    p = str(tmp_path / "a.fsvi")
    b.finish(p).close()
    assert open(p, "rb").read() == ref.finish()


@pytest.mark.parametrize("dim,on_device", [(7, False), (33, False), (33, True), (8, True)])
def test_refusals_of_rows_that_are_not_16_byte_aligned(tmp_path, dim, on_device):
    """The ingest variant with 4-byte loads (dim % 4 != 0, or a device pointer off the 16-byte grid: dim 8 from an odd element) gives
    the same verdicts and names the same rows as the 16-byte one: rows in the first, second and third wave, first and last column."""
    import torch
    fa = _fa()
    rng = np.random.default_rng(40 + dim)
    n = 150
    good = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"u{i}" for i in range(n)]
    b = fa.IndexBuilder(dim, "emb", "r1", quantization=1, chunk_rows=37)
    ref = R.Builder(dim, "f16", "emb", "r1", 0, chunk_rows=37)
    keep = []

    def add(rows):
        if not on_device:
            return b.add(ids, rows)
        t = torch.zeros(n * dim + 1, dtype=torch.float32, device="cuda:0")   # element 1: 4 bytes past a 16-byte boundary
        t[1:] = torch.from_numpy(np.ascontiguousarray(rows)).reshape(-1).to("cuda:0")
        torch.cuda.synchronize()
        keep.append(t)
        assert (t.data_ptr() + 4) % 16 == 4
        return b.add_device(ids, t.data_ptr() + 4)

    for row, col, val, rule in ((0, 0, np.nan, "nonfinite"), (63, dim - 1, np.inf, "nonfinite"), (64, dim // 2, -np.inf, "nonfinite"),
                                (149, dim - 1, np.nan, "nonfinite"), (128, None, 0.0, "norm"), (65, None, 2.0e19, "norm")):
        bad = good.copy()
        if col is None:
            bad[row] = val
        else:
            bad[row, col] = val
        if row + 2 < n:
            bad[row + 2, 0] = np.nan   # a later offender does not change the answer
        with pytest.raises(fa.InvalidConfig) as err:
            add(bad)
        assert R.RULES[rule] in str(err.value), str(err.value)
        assert err.value.bad_row == row and b.record_count() == 0
    add(good)
    ref.add(ids, good)
    p = str(tmp_path / "a.fsvi")
    b.finish(p).close()
    assert open(p, "rb").read() == ref.finish()


def test_a_failed_staging_allocation_leaves_the_builder_whole(tmp_path):
    """A staging chunk that cannot be allocated (one chunk of 2^32 - 1 rows of 4 KiB is beyond any card) is a device error of the add:
    nothing is staged, no row is named, the call may be repeated with the same answer, and the builder still finishes what it holds."""
    from frankensearch_amd.errors import DeviceError
    fa = _fa()
    dim = 1024
    v = np.ones((3, dim), F32)
    b = fa.IndexBuilder(dim, "emb", "r1", quantization=0, chunk_rows=0xFFFFFFFF)
    for _ in range(2):
        with pytest.raises(DeviceError) as err:
            b.add(["a", "b", "c"], v)
        assert err.value.bad_row is None and b.record_count() == 0
    with pytest.raises(DeviceError):
        fa.IndexBuilder(dim, "emb", "r1", quantization=0, chunk_rows=0xFFFFFFFF, reserve_rows=1)
    p, w = str(tmp_path / "a.fsvi"), str(tmp_path / "w.fsvi")
    idx = b.finish(p)
    assert idx.record_count() == 0 and b.last_stats.chunks == 0
    assert fa._lib.lib().fsgpu_fsvi_write_quant(w.encode(), b"emb", b"r1", dim, 0, None, None, None, 0, 0, 0) == 0
    assert open(p, "rb").read() == open(w, "rb").read()
    idx.close()


@pytest.mark.parametrize("dim", [8, 100, 384])
def test_boundary_and_underflow_verdicts_are_the_restatements(dim):
    """Rows whose norm_sq lies at FLT_MAX: whether the f32 sum is finite depends on the order of the additions, and the order is the
    reference's.  Row for row, one add each."""
    fa = _fa()
    rows = R.boundary_fixture(dim, 1000 + dim)
    zero, tiny = R.underflow_pair(dim)
    rows = np.concatenate([rows, zero, tiny], axis=0)
    want = R.row_verdicts(rows)
    assert want[-2:] == ["norm", None] and 8 <= sum(w is None for w in want[:-2]) <= len(want) - 10
    b = fa.IndexBuilder(dim, "emb", "", quantization=0)
    got = []
    for i, r in enumerate(rows):
        try:
            b.add([f"r{i}"], r[None, :])
            got.append(None)
        except fa.InvalidConfig as e:
            assert e.bad_row == 0
            got.append("norm" if R.RULES["norm"] in str(e) else str(e))
    assert got == want
    assert b.record_count() == sum(w is None for w in want)
    # ... and as one call: the first refused row is named
    with pytest.raises(fa.InvalidConfig) as err:
        fa.IndexBuilder(dim, "emb", "").add([f"r{i}" for i in range(len(rows))], rows)
    assert err.value.bad_row == want.index("norm")


def test_special_values_arrive_in_the_slab(tmp_path):
    fa = _fa()
    dim = 33
    v = np.ones((len(R.SPECIALS) + 1, dim), F32)
    for i, s in enumerate(R.SPECIALS):
        v[i, 1 + i % (dim - 1)] = s
        v[i, 0] = -s
    v[-1, :20] = R.SPECIALS
    ids = [f"s{i}" for i in range(len(v))]
    for quant in ("f16", "f32"):
        _, idx = _build(fa, ids, v, dim, quant, 5, None)
        order = sorted(range(len(ids)), key=lambda i: CR.sort_key(ids[i]))
        with np.errstate(over="ignore"):
            want = v.astype("<f2").astype(F32) if quant == "f16" else v
        for r, src in enumerate(order):
            assert idx.doc_id_at(r) == ids[src]
            assert np.array_equal(bits(idx.vector_at(r)), bits(want[src])), (quant, r)
        if quant == "f16":
            assert np.isinf(want).any() and (np.abs(want[want != 0]) < 6.2e-5).any()   # beyond 65,504 -> inf; f16 subnormals kept
        else:
            assert np.any(bits(want) == 0x80000000)   # -0.0 kept
        idx.close()


def test_duplicate_rule_spent_builder_and_unwritable_path(tmp_path):
    fa = _fa()
    dim = 7
    rng = np.random.default_rng(9)
    v = rng.standard_normal((6, dim)).astype(F32)
    # off: duplicates are kept in arrival order (the writer's stable sort)
    b = fa.IndexBuilder(dim, "emb", "r1")
    b.add(["a", "b", "a"], v[:3])
    b.add(["a"], v[3:4])
    idx = b.finish(None)
    got = [(idx.doc_id_at(r), bits(idx.vector_at(r)).tolist()) for r in range(4)]
    with np.errstate(over="ignore"):
        enc = v.astype("<f2").astype(F32)
    want = sorted([("a", 0), ("b", 1), ("a", 2), ("a", 3)], key=lambda t: CR.sort_key(t[0]))
    assert got == [(d, bits(enc[i]).tolist()) for d, i in want]
    idx.close()
    # on: a doc id already staged, or repeated inside the call
    b = fa.IndexBuilder(dim, "emb", "r1", reject_duplicates=True)
    b.add(["a", "b"], v[:2])
    _refused(fa, b, ["c", "a"], v[2:4], "duplicate", 1)
    _refused(fa, b, ["c", "d", "d"], v[2:5], "duplicate", 2)
    b.add(["c", "d"], v[2:4])          # (the refused calls left no trace of "c" or "d")
    _refused(fa, b, ["c"], v[4:5], "duplicate", 0)
    assert b.record_count() == 4
    # a finish into an unwritable path fails and leaves the builder whole; then it succeeds into a good one
    with pytest.raises(fa.IoError):
        b.finish(str(tmp_path / "no-such-dir" / "a.fsvi"))
    assert b.record_count() == 4
    b.add(["e"], v[4:5])
    p = str(tmp_path / "a.fsvi")
    idx = b.finish(p)
    ids = ["a", "b", "c", "d", "e"]
    fa.write_fsvi(str(tmp_path / "w.fsvi"), list(zip(ids, v[[0, 1, 2, 3, 4]])), "emb", "r1")
    assert open(p, "rb").read() == open(str(tmp_path / "w.fsvi"), "rb").read()
    # a finished builder is spent
    assert b.record_count() == 5
    with pytest.raises(fa.InvalidConfig, match="finished"):
        b.add(["f"], v[5:6])
    with pytest.raises(fa.InvalidConfig, match="finished"):
        b.finish(None)
    with pytest.raises(fa.InvalidConfig, match="finished"):
        b.add_device(["f"], 0)
    idx.close()
    b.close()


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_writes_after_finish_work_as_on_an_opened_file(tmp_path, quant):
    fa = _fa()
    dim, n = 43, 300
    rng = np.random.default_rng(21)
    v = rng.standard_normal((n, dim)).astype(F32)
    ids = [f"doc-{i:04d}" for i in range(n)]
    ids[200] = ids[10]
    p = str(tmp_path / "a.fsvi")
    _, built = _build(fa, ids, v, dim, quant, 64, p, gen=1)
    opened = fa.VectorIndex.open(p)
    m = CR.Model(list(zip(ids, v)), dim, quant, 1, "emb", "r1")
    writes = [("doc-0005", rng.standard_normal(dim).astype(F32)), ("new-1", rng.standard_normal(dim).astype(F32)),
              (ids[10], rng.standard_normal(dim).astype(F32)), ("new-1", rng.standard_normal(dim).astype(F32))]
    queries = rng.standard_normal((3, dim)).astype(F32)
    for h in (built, opened):
        h.append_batch(writes)
        assert h.soft_delete("doc-0007") and not h.soft_delete("never")
    m.append_batch(writes)
    m.soft_delete("doc-0007")
    _assert_same_handle(built, opened, queries)
    for h, name in ((built, "cb.fsvi"), (opened, "co.fsvi")):
        st = h.compact(str(tmp_path / name))
        assert (st.main_records_before, st.wal_records) == (n, len(m.wal))
    m.compact()
    assert open(str(tmp_path / "cb.fsvi"), "rb").read() == open(str(tmp_path / "co.fsvi"), "rb").read() == m.image()
    _assert_same_handle(built, opened, queries)
    for d in ids[20:120]:
        m.soft_delete(d)
        for h in (built, opened):
            h.soft_delete(d)
    assert built.needs_vacuum() and opened.needs_vacuum() and m.needs_vacuum()
    for h, name in ((built, "vb.fsvi"), (opened, "vo.fsvi")):
        st = h.vacuum(str(tmp_path / name))
        assert st.tombstones_removed == 100
    m.vacuum()
    assert open(str(tmp_path / "vb.fsvi"), "rb").read() == open(str(tmp_path / "vo.fsvi"), "rb").read() == m.image()
    _assert_same_handle(built, opened, queries)
    built.close()
    opened.close()


def _fnv1a_fixed(ids_bytes):
    """FNV-1a 64 of n ids of one length, [n, len] uint8 -> [n] uint64."""
    h = np.full(ids_bytes.shape[0], 0xCBF29CE484222325, dtype=np.uint64)
    with np.errstate(over="ignore"):
        for j in range(ids_bytes.shape[1]):
            h = (h ^ ids_bytes[:, j].astype(np.uint64)) * np.uint64(0x100000001B3)
    return h


def test_offsets_are_64_bit():
    """Source, staging (one chunk) and final slab each exceed 2^32 bytes: F32, dim 1024, 1,050,000 rows generated on the device."""
    import torch
    fa = _fa()
    n, dim = 1_050_000, 1024
    row_bytes = dim * 4
    assert n * row_bytes > 2 ** 32 and 2 ** 32 // row_bytes == 1 << 20
    dev = torch.device("cuda", 0)
    src = torch.empty((n, dim), dtype=torch.float32, device=dev)
    assert fa._lib.lib().fsgpu_bench_fixture_device(0, 0, n, dim, 64, 0.35, 1, 0, src.data_ptr(), None) == 0
    id_bytes = np.frombuffer(b"".join(b"%07d" % i for i in range(n)), dtype=np.uint8).reshape(n, 7)
    ids = [bytes(r) for r in id_bytes]
    h = _fnv1a_fixed(id_bytes)
    assert int(h[123]) == CR.fnv1a64(b"0000123")
    order = np.lexsort((np.arange(n), h))   # (equal lengths, distinct ids: hash ties would need the bytes — there are none)
    assert np.unique(h).size == n
    b = fa.IndexBuilder(dim, "emb", "r1", quantization=0, chunk_rows=1_100_000)
    b.add_device(ids, src.data_ptr())
    assert b.record_count() == n
    idx = b.finish(None)
    st = b.last_stats
    assert st.ingest_launches == 2 and st.permute_launches == 2 and st.chunks == 1
    assert st.peak_device_bytes >= 1_100_000 * row_bytes + n * row_bytes + n * 4
    edge = 2 ** 32 // row_bytes
    inverse = np.empty(n, dtype=np.int64)
    inverse[order] = np.arange(n)
    file_rows = {0, 1, n - 2, n - 1, edge - 1, edge, edge + 1}                       # file space
    file_rows |= {int(inverse[p]) for p in (0, 1, n - 2, n - 1, edge - 1, edge, edge + 1)}   # arrival space
    file_rows |= set(np.random.default_rng(1).integers(0, n, 256).tolist())
    sample = np.array(sorted(file_rows))
    want = src[torch.from_numpy(order[sample]).to(dev)].cpu().numpy()
    for r, w in zip(sample, want):
        assert idx.doc_id_at(int(r)) == ids[int(order[r])].decode(), int(r)
        assert np.array_equal(bits(idx.vector_at(int(r))), bits(w)), int(r)
    idx.close()
    b.close()
    del src
    torch.cuda.empty_cache()


def test_two_tier_index_builder(tmp_path):
    """The finished pair answers SyncTwoTierSearcher.search as the pair built through write_fsvi + open does."""
    from oracle import bert_oracle
    from frankensearch_amd.two_tier import POOL_RESCORED, SyncTwoTierSearcher, TwoTierConfig, TwoTierIndex, TwoTierIndexBuilder
    fa = _fa()
    rng = np.random.default_rng(31)
    n = 600
    ids = [f"doc-{i:05d}" for i in range(n)]
    fast = rng.standard_normal((n, 256)).astype(F32)
    qual = rng.standard_normal((n, 128)).astype(F32)
    tb = TwoTierIndexBuilder(chunk_rows=97, batch=250)
    with pytest.raises(fa.InvalidConfig, match="at least one fast-tier record is required"):
        TwoTierIndexBuilder().finish()
    for i in range(n):
        if i % 3 == 0:
            tb.add_record(ids[i], fast[i], qual[i])
        else:
            tb.add_fast_record(ids[i], fast[i])
            tb.add_quality_record(ids[i], qual[i])
    with pytest.raises(fa.InvalidConfig, match="duplicate doc_id in fast tier"):
        tb.add_fast_record(ids[3], fast[3])
    with pytest.raises(fa.InvalidConfig, match="duplicate doc_id in quality tier"):
        tb.add_record("fresh", fast[3], qual[3])   # (the fast record of "fresh" is in; its quality id is new, so this one passes ...)
        tb.add_quality_record("fresh", qual[3])    # ... and this one is the duplicate
    with pytest.raises(fa.DimensionMismatch):
        tb.add_fast_record("other", fast[0][:100])
    d = tmp_path / "pair"
    d.mkdir()
    pair = tb.finish(str(d))
    assert sorted(os.listdir(d)) == ["vector.fast.idx", "vector.quality.idx"]
    all_ids, all_fast, all_qual = ids + ["fresh"], np.concatenate([fast, fast[3:4]]), np.concatenate([qual, qual[3:4]])
    pf, pq = str(tmp_path / "f.fsvi"), str(tmp_path / "q.fsvi")
    fa.write_fsvi(pf, list(zip(all_ids, all_fast)), "fast-tier", "")
    fa.write_fsvi(pq, list(zip(all_ids, all_qual)), "quality-tier", "")
    assert open(str(d / "vector.fast.idx"), "rb").read() == open(pf, "rb").read()
    assert open(str(d / "vector.quality.idx"), "rb").read() == open(pq, "rb").read()
    wf, wq = fa.VectorIndex.open(pf), fa.VectorIndex.open(pq)
    assert pair.alignment_kind() == TwoTierIndex(wf, wq).alignment_kind()
    m2v = fa.Model2VecEmbedder(rng.standard_normal((1000, 256)).astype(F32))
    bert = fa.NativeEmbedder(bert_oracle.random_weights(5, 500, 128, 2, 512))
    for pool in (0, POOL_RESCORED):
        cfg = TwoTierConfig(quality_pool=pool)
        a = SyncTwoTierSearcher(pair.fast, pair.quality, m2v, bert, pair.fast.doc_id_at, cfg)
        w = SyncTwoTierSearcher(wf, wq, m2v, bert, wf.doc_id_at, cfg)
        for trial in range(3):
            ft = rng.integers(1, 1000, 9).tolist()
            qt = [101] + rng.integers(1, 500, 12).tolist() + [102]
            oa, ow = a.search(ft, qt, 10), w.search(ft, qt, 10)
            assert oa.fast_hits == ow.fast_hits and oa.quality_hits == ow.quality_hits and oa.blended == ow.blended
            assert oa.initial_results == ow.initial_results and oa.final_results == ow.final_results
    # a directory-less finish gives the same pair
    tb2 = TwoTierIndexBuilder()
    tb2.add_fast_records(all_ids, all_fast)
    tb2.add_quality_records(all_ids, all_qual)
    pair2 = tb2.finish()
    for r in (0, 1, 300, n):
        assert pair2.fast.doc_id_at(r) == wf.doc_id_at(r) and np.array_equal(bits(pair2.quality.vector_at(r)), bits(wq.vector_at(r)))


def test_a_fast_only_pair_and_a_refused_batch(tmp_path):
    """Without a quality record finish() gives a fast-only pair: what needs a quality tier says so instead of reaching the library.
    A batch the device builder refuses is dropped whole, and the builder goes on."""
    from frankensearch_amd.two_tier import TwoTierIndex, TwoTierIndexBuilder
    fa = _fa()
    rng = np.random.default_rng(77)
    v = rng.standard_normal((9, 16)).astype(F32)
    tb = TwoTierIndexBuilder(batch=4)
    tb.add_fast_records(["a", "b", "c"], v[:3])
    bad = v[3:6].copy()
    bad[1, 2] = np.nan
    with pytest.raises(fa.InvalidConfig, match="all embedding values must be finite") as err:
        tb.add_fast_records(["d", "e", "f"], bad)      # the fourth record fills the batch: "a" .. "f" go to the device, row 4 is refused
    assert err.value.bad_row == 4
    tb.add_fast_records(["a", "b", "c", "d", "e", "f"], v[:6])   # dropped whole: none of the ids is taken
    pair = tb.finish(str(tmp_path))
    assert sorted(os.listdir(tmp_path)) == ["vector.fast.idx"]
    assert not pair.has_quality_index() and pair.quality is None and pair.alignment_kind() == TwoTierIndex.NONE
    assert sorted(pair.fast.doc_id_at(r) for r in range(pair.fast.record_count())) == ["a", "b", "c", "d", "e", "f"]
    for call in (lambda: pair.quality_row(0), pair.unmatched_quality_docs, lambda: pair.quality_scores_for_hits(v[0], [("a", 1.0, 0)]),
                 lambda: pair.quality_scores_for_hits_batched(v[:1], [[("a", 1.0, 0)]]), lambda: pair.mmr_rerank([("a", 1.0, 0)], None)):
        with pytest.raises(fa.InvalidConfig, match="no quality tier"):
            call()
    pair.close()

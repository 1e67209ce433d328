"""CPU-side contract of the index builder: tests/index_build_ref.py (the restatement the GPU tests compare the library with) is pinned
against compaction_ref's image and the oracle's FSVI writer, the fixtures are shown to have the properties the GPU tests rely on —
the boundary rows really are order-sensitive, the underflow pair behaves as stated, and every fault of a fixed list changes a verdict
or a file byte of them — and the new C ABI entry points answer with a status, not a crash, on a host without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compaction_ref as CR  # noqa: E402
import index_build_ref as R  # noqa: E402

BOUNDARY_DIMS = (8, 100, 384)


def built(dim, n, chunk, quant, seed, fault=None, **kw):
    ids, v = R.fixture(dim, n, seed)
    b = R.Builder(dim, quant, "emb", "r1", 3, chunk_rows=chunk or 65536, fault=fault, **kw)
    for lo, hi in R.split_adds(n):
        b.add(ids[lo:hi], v[lo:hi])
    return b, ids, v


@pytest.mark.parametrize("case", list(enumerate(R.cases())), ids=lambda c: "%d-dim%d-n%d-chunk%d-%s" % ((c[0],) + c[1]))
def test_restated_image_equals_compaction_ref_and_the_oracle_writer(oracle, tmp_path, case):
    seed, (dim, n, chunk, quant) = case
    b, ids, v = built(dim, n, chunk, quant, seed)
    image = b.finish()
    m = CR.Model(list(zip(ids, v)), dim, quant, gen=3, embedder_id="emb", revision="r1")
    assert image == m.image()
    if n:   # (the oracle's writer takes at least one record)
        p = str(tmp_path / "o.fsvi")
        assert oracle.fsvi_write(p, [(d, row) for d, row in zip(ids, v)], "emb", "r1", 3, 1 if quant == "f16" else 0) == 0
        assert open(p, "rb").read() == image


def test_the_cases_cover_the_matrix():
    cs = R.cases()
    assert {(d, n) for d, n, _, _ in cs} == {(d, n) for d in R.DIMS for n in R.NS}
    for d in R.DIMS:
        assert {q for dd, _, _, q in cs if dd == d} == {"f16", "f32"}
        assert {c for dd, _, c, _ in cs if dd == d} == set(R.CHUNKS)
    assert R.split_adds(5000) == [(0, 1), (1, 65), (65, 194), (194, 5000)] and R.split_adds(0) == [] and R.split_adds(64) == [(0, 1), (1, 64)]
    ids, _ = R.fixture(8, 1000, 0)
    assert "" in ids and "x" * 65535 in ids and len(set(ids)) == len(ids) - 2
    for a, b in R.COLLIDING:
        assert a != b and CR.fnv1a64(a.encode()) == CR.fnv1a64(b.encode()) and ids.index(a) < ids.index(b) and a.encode() > b.encode()


@pytest.mark.parametrize("dim", BOUNDARY_DIMS)
def test_boundary_fixture_is_order_sensitive(dim):
    rows = R.boundary_fixture(dim, 1000 + dim)
    assert rows.shape == (48, dim) and rows.dtype == np.float32 and np.all(np.isfinite(rows))
    exact = np.array([float(np.sum(r.astype(np.float64) ** 2)) for r in rows])
    assert np.all(np.abs(exact / R.FLT_MAX - 1.0) <= 2.0 ** -23)
    seq, pair = np.isfinite(R.norm_sq_sequential(rows)), np.isfinite(R.norm_sq_pairwise(rows))
    assert int(np.sum(seq != pair)) >= 8, (int(np.sum(seq != pair)), int(np.sum(seq)), int(np.sum(pair)))
    # the sequential sum itself, element by element in numpy scalars: the vectorised form above is the same arithmetic
    for r in rows[:6]:
        acc = np.float32(0)
        with np.errstate(over="ignore"):
            for x in r:
                acc = np.float32(acc + np.float32(x * x))
        assert np.isfinite(acc) == np.isfinite(R.norm_sq_sequential(r[None, :])[0])


@pytest.mark.parametrize("dim", (1, 8, 100, 384))
def test_underflow_pair(dim):
    zero, tiny = R.underflow_pair(dim)
    assert R.row_verdicts(zero) == ["norm"] and R.norm_sq_sequential(zero)[0] == 0.0
    assert R.row_verdicts(tiny) == [None]
    s = float(R.norm_sq_sequential(tiny)[0])
    assert 0.0 < s < R.FLT_MIN_NORMAL   # a subnormal sum
    if dim == 384:
        assert abs(s - 5.38e-43) < 0.01e-43
    b = R.Builder(dim)
    with pytest.raises(R.Refused) as err:
        b.add(["ok", "z"], np.concatenate([tiny, zero]))
    assert (err.value.status, err.value.rule, err.value.row) == ("InvalidConfig", "norm", 1) and b.record_count() == 0
    b.add(["ok"], tiny)
    assert b.record_count() == 1


def test_validation_order_and_all_or_nothing():
    b = R.Builder(4, reject_duplicates=True)
    good = np.ones((3, 4), np.float32)
    b.add(["a", "b", "c"], good)
    bad = good.copy()
    bad[2, 1] = np.inf
    for ids, v, want in ((["d", "a", "e"], good, ("duplicate", 1)), (["d", "e", "e"], good, ("duplicate", 2)),
                         (["d", "y" * 65536, "a"], good, ("doc_id_len", 1)), (["d", "a", "e"], bad, ("duplicate", 1)),
                         (["d", "e", "a"], bad, ("nonfinite", 2)), (["d", "e", "f"], np.zeros((3, 4), np.float32), ("norm", 0))):
        with pytest.raises(R.Refused) as err:
            b.add(ids, v)
        assert (err.value.rule, err.value.row) == want
        assert b.record_count() == 3
    with pytest.raises(R.Refused) as err:
        b.add(["q"], np.ones((1, 5), np.float32))
    assert err.value.status == "DimensionMismatch"
    b.add(["", "y" * 65535], good[:2])   # the empty id and the longest id are legal
    assert b.record_count() == 5


@pytest.mark.parametrize("fault", R.FAULTS)
def test_every_fault_shows_on_the_fixtures(fault):
    """A fault put in place of the restatement changes a verdict of the boundary / underflow fixtures or the file bytes of a case."""
    shown = []
    for dim in BOUNDARY_DIMS:
        rows = R.boundary_fixture(dim, 1000 + dim)
        if R.row_verdicts(rows, fault) != R.row_verdicts(rows):
            shown.append(("boundary", dim))
        for part in R.underflow_pair(dim):
            if R.row_verdicts(part, fault) != R.row_verdicts(part):
                shown.append(("underflow", dim))
    if not shown:
        for seed, (dim, n, chunk, quant) in enumerate(R.cases()):
            if n * dim > 200000:   # (the small cases are enough to show a fault, and quick)
                continue
            if built(dim, n, chunk, quant, seed, fault)[0].finish() != built(dim, n, chunk, quant, seed)[0].finish():
                shown.append(("bytes", dim, n, chunk, quant))
                break
    assert shown, fault


def test_new_entry_points_answer_with_a_status_without_a_gpu():
    import torch
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    from frankensearch_amd.index_builder import _Options

    build()
    L = _lib.lib()
    h = C.c_void_p()
    # option values are judged before a device is looked for
    for bad in (_Options(quantization=2), _Options(quantization=1, compaction_gen=256), _Options(quantization=1, reject_duplicates=2),
                _Options(1, 0, 0, 0, 0, (C.c_uint32 * 6)(0, 0, 0, 0, 0, 7))):
        assert L.fsgpu_index_builder_create(0, 8, b"e", b"", C.byref(bad), C.byref(h)) == _lib.ERR_INVALID_CONFIG and not h.value
    assert L.fsgpu_index_builder_create(0, 0, b"e", b"", None, C.byref(h)) == _lib.ERR_INVALID_CONFIG
    assert L.fsgpu_index_builder_create(0, 8, None, b"", None, C.byref(h)) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_builder_create(0, 8, b"e", b"", None, None) == _lib.ERR_NULL_ARGUMENT
    bad_row = C.c_uint64(77)
    assert L.fsgpu_index_builder_add(None, 1, None, None, None, 8, C.byref(bad_row)) == _lib.ERR_NULL_ARGUMENT and bad_row.value == 77
    assert L.fsgpu_index_builder_finish(None, None, C.byref(h), None) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_builder_record_count(None) == 0
    L.fsgpu_index_builder_destroy(None)
    if not torch.cuda.is_available():
        import frankensearch_amd as fa
        assert L.fsgpu_index_builder_create(0, 8, b"e", b"", None, C.byref(h)) == _lib.ERR_NO_DEVICE and not h.value
        with pytest.raises(fa.NoDevice):
            fa.IndexBuilder(8)
        with pytest.raises(fa.InvalidConfig):
            fa.TwoTierIndexBuilder().finish()

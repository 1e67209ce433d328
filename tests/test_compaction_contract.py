"""CPU-side contract of compaction and vacuum: tests/compaction_ref.py (the restatement the GPU tests compare the library with) is
pinned with the reference's own test literals and against the oracle's FSVI writer, the properties the GPU tests rely on are
asserted, and the new C ABI entry points answer with a status — not a crash — on a host without a GPU."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import compaction_ref as R  # noqa: E402


def sample_vector(x, dim):
    """lib.rs test helper sample_vector: every component the same value."""
    return [x] * dim


def test_needs_compaction_threshold():
    # lib.rs:9771-9800 (needs_compaction_threshold): 10 main rows, threshold 5, ratio 0.10
    m = R.Model([(f"main-{i}", sample_vector(0.1, 4)) for i in range(10)], 4)
    assert not m.needs_compaction(5, 0.10)
    m.append("wal-0", sample_vector(0.2, 4))   # ratio = 1/10 = 0.10: hits the ratio threshold
    assert m.needs_compaction(5, 0.10)


def test_set_wal_config_overrides_defaults():
    # lib.rs:10700-10727
    m = R.Model([(f"d{i}", sample_vector(0.1, 4)) for i in range(100)], 4)
    m.append("wal-1", sample_vector(0.5, 4))
    assert not m.needs_compaction()            # 1 / 100 < 0.10 and 1 < 1000
    assert m.needs_compaction(1, 0.001)
    assert m.needs_compaction(1000, float("nan")) is False   # NaN ratio -> 0.10 (lib.rs:2280-2286)
    m2 = R.Model([(f"d{i}", sample_vector(0.1, 4)) for i in range(10)], 4)
    m2.append("w", sample_vector(0.5, 4))
    assert m2.needs_compaction(1000, float("nan"))           # 1 / 10 >= 0.10


def test_compact_preserves_wal_config():
    # lib.rs:10861-10891: 20 rows, threshold 99, ratio 0.90
    m = R.Model([(f"d{i}", sample_vector(0.1, 4)) for i in range(20)], 4)
    m.append("wal-1", sample_vector(0.5, 4))
    m.compact()
    assert len(m.wal) == 0 and m.record_count() == 21
    m.append("wal-2", sample_vector(0.3, 4))
    assert not m.needs_compaction(99, 0.90)    # 1 / 21 ~ 0.048 < 0.90


def test_compaction_merges_wal_into_main():
    # lib.rs:9732-9768
    m = R.Model([("main-0", [1.0, 0.0, 0.0, 0.0])], 4)
    m.append("wal-0", [0.0, 1.0, 0.0, 0.0])
    m.append("wal-1", [0.0, 0.0, 1.0, 0.0])
    assert m.record_count() == 1 and len(m.wal) == 2
    st = m.compact()
    assert st == {"main_records_before": 1, "wal_records": 2, "total_records_after": 3}
    assert m.record_count() == 3 and len(m.wal) == 0


def test_tombstone_ratio_and_needs_vacuum_threshold():
    # lib.rs:8893-8918: the threshold is strictly greater-than
    m = R.Model([(f"doc-{i}", sample_vector(0.1, 4)) for i in range(10)], 4)
    assert not m.needs_vacuum()
    m.soft_delete("doc-0")
    m.soft_delete("doc-1")
    assert m.tombstone_count() == 2 and not m.needs_vacuum()
    m.soft_delete("doc-2")
    assert m.tombstone_count() == 3 and m.needs_vacuum()


def test_vacuum_removes_tombstones():
    # lib.rs:8921-8962, and vacuum_noop_when_no_tombstones :9291
    m = R.Model([("doc-a", [1.0, 0, 0, 0]), ("doc-b", [0, 1.0, 0, 0]), ("doc-c", [0, 0, 1.0, 0])], 4, embedder_id="fnv1a-384")
    assert m.vacuum()["tombstones_removed"] == 0
    m.soft_delete("doc-b")
    st = m.vacuum()
    assert (st["records_before"], st["records_after"], st["tombstones_removed"]) == (3, 2, 1) and st["bytes_reclaimed"] > 0
    assert m.record_count() == 2 and m.tombstone_count() == 0 and all(d != "doc-b" for d, _ in m.rows())


def test_next_generation_wraps_past_zero():
    assert [R.next_generation(g) for g in (0, 1, 254, 255)] == [1, 2, 255, 1]


def _strictly_increasing(rows):
    keys = [R.sort_key(d) for d, _ in rows]
    return all(a < b for a, b in zip(keys, keys[1:]))


def test_properties_the_gpu_tests_rely_on():
    rng = np.random.default_rng(5)
    dim = 8
    vec = lambda: rng.standard_normal(dim).astype(np.float32)   # noqa: E731
    rows = [(f"doc-{i:03d}", vec()) for i in range(200)] + [("twin", vec()), ("twin", vec())]
    twin_second = R.encode_row(rows[-1][1], "f16")
    m = R.Model(rows, dim)
    # compact with an empty WAL leaves tombstones (lib.rs:2740-2747)
    m.soft_delete("doc-007")
    st = m.compact()
    assert st == {"main_records_before": 202, "wal_records": 0, "total_records_after": 202}
    assert m.tombstone_count() == 1 and m.gen == 1
    # WAL beats main; the last live main duplicate wins; the output is strictly increasing in (hash, id)
    new = vec()
    m.append("doc-100", new)
    m.append("fresh", vec())
    m.append_batch([("rep", vec()), ("rep", vec()), ("rep", np.ones(dim, np.float32))])
    assert [d for d, _ in m.wal] == ["doc-100", "fresh", "rep"] and np.all(m.wal[-1][1] == 1.0)
    st = m.compact()
    out = dict(m.rows())
    assert _strictly_increasing(m.rows()) and len(out) == len(m.rows()) == st["total_records_after"] == 202 - 1 - 1 + 2
    assert out["doc-100"] == R.encode_row(new, "f16") and "doc-007" not in out
    assert out["twin"] == twin_second and out["rep"] == R.encode_row(np.ones(dim), "f16")
    assert m.gen == 2 and m.tombstone_count() == 0 and not m.wal
    # an appended doc id that is twice live in the file: the FIRST is tombstoned by the append, the WAL entry wins over the second
    m2 = R.Model(rows, dim)
    m2.append("twin", new)
    assert [r[2] for r in m2.main if r[0] == "twin"] == [True, False]
    m2.compact()
    assert dict(m2.rows())["twin"] == R.encode_row(new, "f16") and _strictly_increasing(m2.rows())
    # a batch with one bad entry changes nothing
    m3 = R.Model(rows, dim)
    with pytest.raises(ValueError):
        m3.append_batch([("ok", vec()), ("bad", [np.inf] + [0.0] * (dim - 1))])
    with pytest.raises(ValueError):
        m3.append_batch([("ok", vec()), ("zero", [0.0] * dim)])
    assert not m3.wal and m3.tombstone_count() == 0
    # vacuum keeps the WAL and the generation, and drops exactly the tombstoned rows in order
    m3.append("doc-001", vec())
    keep = [(r[0], r[1]) for r in m3.main if not r[2]]
    st = m3.vacuum()
    assert m3.rows() == keep and len(m3.wal) == 1 and m3.gen == 1 and st["tombstones_removed"] == 1
    assert st["bytes_reclaimed"] == R.fsvi_image_len(202, sum(len(d) for d, _ in rows), dim, "f16", "hash", "test") - m3.image_len()


@pytest.mark.parametrize("quant", ["f16", "f32"])
def test_restated_image_equals_the_oracle_writer(oracle, tmp_path, quant):
    rng = np.random.default_rng(11)
    dim = 43
    rows = [(f"id-{i}", rng.standard_normal(dim).astype(np.float32)) for i in range(57)] + [("id-3", rng.standard_normal(dim).astype(np.float32))]
    m = R.Model(rows, dim, quant, gen=7, embedder_id="emb", revision="r1")
    p = str(tmp_path / "a.fsvi")
    assert oracle.fsvi_write(p, [(d, v.tolist()) for d, v in rows], "emb", "r1", 7, 1 if quant == "f16" else 0) == 0
    assert open(p, "rb").read() == m.image()
    # ... and of the rows a compaction leaves, handed back to the writer as widened values
    m.append("id-5", rng.standard_normal(dim).astype(np.float32))
    m.append("zz", rng.standard_normal(dim).astype(np.float32))
    m.compact()
    assert oracle.fsvi_write(p, [(d, v.tolist()) for d, v in m.writer_rows()], "emb", "r1", m.gen, 1 if quant == "f16" else 0) == 0
    assert open(p, "rb").read() == m.image() and m.gen == 8


def test_new_entry_points_answer_with_a_status_without_a_gpu():
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build

    build()
    L = _lib.lib()
    null = None
    out = C.c_int32(7)
    ids = (C.c_char_p * 1)(b"a")
    lens = (C.c_uint32 * 1)(1)
    vec = (C.c_float * 4)(1, 0, 0, 0)
    assert L.fsgpu_index_compact(null, None, None) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_vacuum(null, b"/nonexistent/x.fsvi", None) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_needs_compaction(null, 1000, 0.1, C.byref(out)) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_needs_vacuum(null, C.byref(out)) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_wal_append_batch(null, 1, C.cast(ids, C.c_void_p), C.cast(lens, C.c_void_p), C.cast(vec, C.c_void_p), 4) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_sharded_compact(null, None, None) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_sharded_vacuum(null, None, None) == _lib.ERR_NULL_ARGUMENT
    assert L.fsgpu_index_tombstone_count(null) == 0 and L.fsgpu_index_live_count(null) == 0
    assert L.fsgpu_index_generation(null) == 0 and L.fsgpu_index_compaction_gen(null) == 0
    assert _lib.last_error()
    import torch
    if not torch.cuda.is_available():
        ms = (C.c_double * 1)()
        assert L.fsgpu_lab_device_copy_ms(0, 1 << 20, 1, ms) == _lib.ERR_NO_DEVICE

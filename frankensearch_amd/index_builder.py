"""IndexBuilder — the device-resident index builder (include/fsgpu.h, "encoder -> index"): VectorIndexWriter::write_record + finish
(crates/frankensearch-index/src/lib.rs:3607-3672, 3752-3943) and the facade's IndexBuilder (frankensearch/src/index_builder.rs:168-264)
for vectors that already sit in device memory.  Batches of (doc id, vector) arrive from host memory, from device memory or straight
from an embedder; they are validated and encoded on the device, and finish() leaves the sorted slab in device memory as a ready
VectorIndex (and the FSVI v1 file when a path is given) — the bytes write_fsvi writes and the handle VectorIndex.open gives.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import _lib
from .errors import SearchError, check
from .index import VectorIndex


class _Options(C.Structure):
    _fields_ = [("quantization", C.c_uint32), ("compaction_gen", C.c_uint32), ("reject_duplicates", C.c_uint32),
                ("chunk_rows", C.c_uint32), ("reserve_rows", C.c_uint64), ("reserved", C.c_uint32 * 6)]


class _Stats(C.Structure):
    _fields_ = [("rows", C.c_uint64), ("chunks", C.c_uint64), ("ingest_launches", C.c_uint64), ("permute_launches", C.c_uint64),
                ("ingest_ms", C.c_double), ("sort_ms", C.c_double), ("permute_ms", C.c_double), ("tables_ms", C.c_double),
                ("file_ms", C.c_double), ("ingest_device_ms", C.c_double), ("permute_device_ms", C.c_double), ("peak_device_bytes", C.c_uint64)]


@dataclass
class IndexBuildStats:
    """fsgpu_index_build_stats."""
    rows: int
    chunks: int
    ingest_launches: int
    permute_launches: int
    ingest_ms: float
    sort_ms: float
    permute_ms: float
    tables_ms: float
    file_ms: float
    ingest_device_ms: float
    permute_device_ms: float
    peak_device_bytes: int


def _doc_id_arrays(doc_ids: Sequence):
    ids = [d if isinstance(d, bytes) else str(d).encode() for d in doc_ids]
    arr = (C.c_char_p * max(len(ids), 1))(*ids)
    lens = np.asarray([len(b) for b in ids], dtype=np.uint32)
    return ids, arr, lens


class IndexBuilder:
    """quantization 1 = F16 (default), 0 = F32.  reject_duplicates: TwoTierIndexBuilder's rule (two_tier.rs:2125-2132); off, duplicate
    ids are kept in arrival order as VectorIndexWriter keeps them.  A refused add stages nothing and raises with `.bad_row` set to the
    index in the call of the first offending row."""

    def __init__(self, dim: int, embedder_id: str = "test", embedder_revision: str = "", device: int = 0, quantization: int = 1,
                 compaction_gen: int = 0, reject_duplicates: bool = False, chunk_rows: int = 0, reserve_rows: int = 0):
        o = _Options(quantization, compaction_gen, int(reject_duplicates), chunk_rows, reserve_rows)
        h = C.c_void_p()
        check(_lib.lib().fsgpu_index_builder_create(device, dim, embedder_id.encode(), embedder_revision.encode(), C.byref(o), C.byref(h)))
        self._h = h
        self._dim = dim
        self.device = device
        self.last_stats: Optional[IndexBuildStats] = None

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_index_builder_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def record_count(self) -> int:
        return _lib.lib().fsgpu_index_builder_record_count(self._h)

    def dimension(self) -> int:
        return self._dim

    @staticmethod
    def _checked(status: int, bad: C.c_uint64) -> None:
        try:
            check(status)
        except SearchError as e:
            e.bad_row = None if bad.value == 0xFFFFFFFFFFFFFFFF else int(bad.value)
            raise

    def add(self, doc_ids: Sequence, vectors) -> None:
        """write_record for a batch: vectors [n, dim] f32 in host memory."""
        v = np.ascontiguousarray(vectors, dtype=np.float32)
        v = v.reshape(len(doc_ids), -1) if len(doc_ids) else v.reshape(0, self._dim)
        ids, arr, lens = _doc_id_arrays(doc_ids)
        bad = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        self._checked(_lib.lib().fsgpu_index_builder_add(self._h, len(ids), C.cast(arr, C.c_void_p), lens.ctypes.data, v.ctypes.data,
                                                         v.shape[1], C.byref(bad)), bad)

    def add_device(self, doc_ids: Sequence, vectors_ptr: int, vector_len: Optional[int] = None, stream: Optional[int] = None) -> None:
        """... [n, vector_len] f32 in memory of the builder's device (a torch tensor's data_ptr(), fsgpu_device_malloc); the ingest is
        enqueued behind `stream` (a hipStream_t as an integer; None = the default stream) and the call returns with the verdict."""
        ids, arr, lens = _doc_id_arrays(doc_ids)
        bad = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        self._checked(_lib.lib().fsgpu_index_builder_add_device(self._h, len(ids), C.cast(arr, C.c_void_p), lens.ctypes.data, vectors_ptr,
                                                                self._dim if vector_len is None else vector_len, stream, C.byref(bad)), bad)

    def add_texts(self, embedder, doc_ids: Sequence, batch: Sequence[Sequence[int]]) -> None:
        """Pre-tokenised texts embedded on the device by a NativeEmbedder or a Model2VecEmbedder and ingested where the embedder left
        them (fsgpu_index_builder_add_bert / _add_m2v).  With a HashEmbedder the batch is a sequence of str (_add_hash)."""
        from .embed import HashEmbedder, Model2VecEmbedder, _text_arrays
        m2v = isinstance(embedder, Model2VecEmbedder)
        n = len(batch)
        if n != len(doc_ids):
            raise ValueError("one doc id per text")
        if isinstance(embedder, HashEmbedder):   # raw texts: a sequence of str (fsgpu_index_builder_add_hash)
            flat, offsets = _text_arrays(batch)
            ids, arr, lens = _doc_id_arrays(doc_ids)
            bad = C.c_uint64(0xFFFFFFFFFFFFFFFF)
            self._checked(_lib.lib().fsgpu_index_builder_add_hash(self._h, embedder._h, flat.ctypes.data, offsets.ctypes.data, n,
                                                                  C.cast(arr, C.c_void_p), lens.ctypes.data, C.byref(bad)), bad)
            return
        offsets = np.zeros(n + 1, dtype=np.uint32)
        for i, t in enumerate(batch):
            offsets[i + 1] = offsets[i] + len(t)
        flat = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint32 if m2v else np.int32)
        for i, t in enumerate(batch):
            flat[offsets[i]:offsets[i + 1]] = np.asarray(t, dtype=flat.dtype)
        ids, arr, lens = _doc_id_arrays(doc_ids)
        bad = C.c_uint64(0xFFFFFFFFFFFFFFFF)
        fn = _lib.lib().fsgpu_index_builder_add_m2v if m2v else _lib.lib().fsgpu_index_builder_add_bert
        self._checked(fn(self._h, embedder._h, flat.ctypes.data, offsets.ctypes.data, n, C.cast(arr, C.c_void_p), lens.ctypes.data,
                         C.byref(bad)), bad)

    def finish(self, path: Optional[str] = None) -> VectorIndex:
        """VectorIndexWriter::finish (lib.rs:3752-3943): the index, and its FSVI v1 image at `path` when one is given.  The builder is
        spent afterwards; a finish that failed may be repeated."""
        h = C.c_void_p()
        st = _Stats()
        check(_lib.lib().fsgpu_index_builder_finish(self._h, None if path is None else str(path).encode(), C.byref(h), C.byref(st)))
        self.last_stats = IndexBuildStats(*(getattr(st, f[0]) for f in _Stats._fields_))
        return VectorIndex(h.value)

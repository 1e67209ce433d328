"""Restatement of the reference's WAL / tombstone bookkeeping over plain Python lists, for the compaction tests.

What it restates (crates/frankensearch-index/src/lib.rs):
  append_batch_impl   :2569-2720   validate all, dedup last-wins keeping order (:2604-2615), supersede resident copies (:2641-2647),
                                   tombstone the first live main row of each doc id (:2667-2711)
  soft_delete_batch   :2303-2397   every main row of the doc id, and its resident WAL entries
  needs_compaction    :2270-2292   needs_vacuum / tombstone_ratio :174, 2464-2475
  compact             :2734-2854   live main rows then WAL entries, STABLE sort by (hash, doc id), adjacent duplicates -> the last
  vacuum              :2485-2521   live main rows in order; WAL and generation kept
  rewrite_index       :2871-3094   main rows as raw bytes, WAL rows encoded (f16 round-to-nearest-even / raw f32), flags cleared
  next_generation     :6156
  write_record + finish :3637-3672, 3752-3943   the FSVI v1 image (header :5714-5768)

A model holds the main rows in FILE order as [doc_id, row bytes, tombstoned] and the resident WAL as [doc_id, f32 vector].
"""
import struct
import zlib

import numpy as np

VACUUM_THRESHOLD = 0.20   # TOMBSTONE_VACUUM_THRESHOLD, lib.rs:174
DEFAULT_COMPACTION_THRESHOLD = 1000
DEFAULT_COMPACTION_RATIO = 0.10


def fnv1a64(b: bytes) -> int:
    h = 0xCBF29CE484222325
    for c in b:
        h = ((h ^ c) * 0x100000001B3) & 0xFFFFFFFFFFFFFFFF
    return h


def sort_key(doc_id: str):
    b = doc_id.encode()
    return (fnv1a64(b), b)


def next_generation(g: int) -> int:
    return 1 if g == 255 else g + 1


def encode_row(vector, quant: str) -> bytes:
    v = np.asarray(vector, dtype=np.float32)
    if quant == "f16":
        return v.astype("<f2").tobytes()   # IEEE round to nearest even, as f16::from_f32
    return v.astype("<f4").tobytes()


def widen_row(raw: bytes, quant: str) -> np.ndarray:
    """The f32 values whose encoding is `raw` again (widening f16 is exact)."""
    return np.frombuffer(raw, dtype="<f2" if quant == "f16" else "<f4").astype(np.float32)


def header_len(embedder_id: str, revision: str) -> int:
    return 4 + 2 + 2 + len(embedder_id.encode()) + 2 + len(revision.encode()) + 4 + 1 + 3 + 8 + 8 + 4


def fsvi_image(rows, dim: int, quant: str, embedder_id: str, revision: str, gen: int, nonce: int = 0) -> bytes:
    """The FSVI v1 image of rows = [(doc_id, row bytes)] already in (hash, doc id) order: header with CRC32, 16-byte records,
    string table, zero padding to 64, slab."""
    eid, rev = embedder_id.encode(), revision.encode()
    strings = b"".join(d.encode() for d, _ in rows)
    pre = header_len(embedder_id, revision) + 16 * len(rows) + len(strings)
    vectors_offset = (pre + 63) // 64 * 64
    head = b"FSVI" + struct.pack("<HH", 1, len(eid)) + eid + struct.pack("<H", len(rev)) + rev
    head += struct.pack("<IBBHQQ", dim, 1 if quant == "f16" else 0, gen, nonce, len(rows), vectors_offset)
    head += struct.pack("<I", zlib.crc32(head) & 0xFFFFFFFF)
    recs, off = b"", 0
    for d, _ in rows:
        b = d.encode()
        recs += struct.pack("<QIHH", fnv1a64(b), off, len(b), 0)
        off += len(b)
    return head + recs + strings + b"\0" * (vectors_offset - pre) + b"".join(r for _, r in rows)


def fsvi_image_len(n: int, strings_len: int, dim: int, quant: str, embedder_id: str, revision: str) -> int:
    pre = header_len(embedder_id, revision) + 16 * n + strings_len
    return (pre + 63) // 64 * 64 + n * dim * (2 if quant == "f16" else 4)


class Model:
    def __init__(self, rows, dim: int, quant: str = "f16", gen: int = 1, embedder_id: str = "hash", revision: str = "test"):
        """rows: (doc_id, f32 vector) as handed to the writer, any order: the writer sorts them stably by (hash, doc id)."""
        self.dim, self.quant, self.gen = dim, quant, gen
        self.embedder_id, self.revision = embedder_id, revision
        order = sorted(range(len(rows)), key=lambda i: sort_key(rows[i][0]))   # sorted() is stable
        self.main = [[rows[i][0], encode_row(rows[i][1], quant), False] for i in order]
        self.wal = []

    # ---- writes ----
    def validate(self, doc_id: str, vector) -> None:
        v = np.asarray(vector, dtype=np.float32).reshape(-1)
        if v.size != self.dim:
            raise ValueError("DimensionMismatch")
        if not np.all(np.isfinite(v)):
            raise ValueError("all embedding values must be finite")
        norm_sq = np.float32(0)
        for x in v:
            norm_sq = np.float32(norm_sq + np.float32(x * x))
        if not (norm_sq > 0 and np.isfinite(norm_sq)):
            raise ValueError("embedding norm must be non-zero and finite")
        if len(doc_id.encode()) > 0xFFFF:
            raise ValueError("doc_id byte length must fit in u16")

    def append_batch(self, entries) -> None:
        entries = list(entries)
        for d, v in entries:   # all of them, before anything changes
            self.validate(d, v)
        seen, kept = set(), []
        for d, v in reversed(entries):
            if d not in seen:
                seen.add(d)
                kept.append((d, np.asarray(v, dtype=np.float32).copy()))
        kept.reverse()
        self.wal = [e for e in self.wal if e[0] not in seen] + [[d, v] for d, v in kept]
        for d, _ in kept:
            for row in self.main:
                if row[0] == d and not row[2]:
                    row[2] = True
                    break

    def append(self, doc_id: str, vector) -> None:
        self.append_batch([(doc_id, vector)])

    def soft_delete(self, doc_id: str) -> bool:
        hit = False
        for row in self.main:
            if row[0] == doc_id and not row[2]:
                row[2] = hit = True
        before = len(self.wal)
        self.wal = [e for e in self.wal if e[0] != doc_id]
        return hit or len(self.wal) != before

    def set_live(self, live) -> None:
        for row, l in zip(self.main, live):
            row[2] = not bool(l)

    # ---- predicates ----
    def record_count(self) -> int:
        return len(self.main)

    def tombstone_count(self) -> int:
        return sum(1 for r in self.main if r[2])

    def needs_compaction(self, threshold: int = DEFAULT_COMPACTION_THRESHOLD, ratio: float = DEFAULT_COMPACTION_RATIO) -> bool:
        if not self.wal:
            return False
        if len(self.wal) >= threshold:
            return True
        if self.main:
            if not np.isfinite(ratio):
                ratio = 0.10
            if len(self.wal) / len(self.main) >= ratio:
                return True
        return False

    def needs_vacuum(self) -> bool:
        return bool(self.main) and self.tombstone_count() / len(self.main) > VACUUM_THRESHOLD

    # ---- rewrites ----
    def image_len(self) -> int:
        return fsvi_image_len(len(self.main), sum(len(r[0].encode()) for r in self.main), self.dim, self.quant, self.embedder_id,
                              self.revision)

    def compact(self) -> dict:
        before, wal_count = len(self.main), len(self.wal)
        if wal_count == 0:
            return {"main_records_before": before, "wal_records": 0, "total_records_after": before}
        sources = [(r[0], r[1]) for r in self.main if not r[2]] + [(d, encode_row(v, self.quant)) for d, v in self.wal]
        sources.sort(key=lambda s: sort_key(s[0]))   # stable
        out = []
        for s in sources:
            if out and out[-1][0] == s[0]:
                out[-1] = s
            else:
                out.append(s)
        self.main = [[d, raw, False] for d, raw in out]
        self.wal = []
        self.gen = next_generation(self.gen)
        return {"main_records_before": before, "wal_records": wal_count, "total_records_after": len(self.main)}

    def vacuum(self, fsvi_opened: bool = True) -> dict:
        before, tomb = len(self.main), self.tombstone_count()
        if before == 0 or tomb == 0:
            return {"records_before": before, "records_after": before, "tombstones_removed": 0, "bytes_reclaimed": 0}
        row_bytes = self.dim * (2 if self.quant == "f16" else 4)
        bytes_before = self.image_len() if fsvi_opened else before * row_bytes
        self.main = [r for r in self.main if not r[2]]
        bytes_after = self.image_len() if fsvi_opened else len(self.main) * row_bytes
        return {"records_before": before, "records_after": len(self.main), "tombstones_removed": before - len(self.main),
                "bytes_reclaimed": max(0, bytes_before - bytes_after)}

    # ---- what is left ----
    def rows(self):
        """(doc_id, row bytes) of every main row, file order."""
        return [(r[0], r[1]) for r in self.main]

    def writer_rows(self):
        """(doc_id, f32 vector) that the FSVI writer turns into exactly these rows again."""
        return [(r[0], widen_row(r[1], self.quant)) for r in self.main]

    def image(self, nonce: int = 0) -> bytes:
        return fsvi_image(self.rows(), self.dim, self.quant, self.embedder_id, self.revision, self.gen, nonce)

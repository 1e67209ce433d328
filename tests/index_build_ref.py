"""Restatement of the index builder's contract in plain numpy / Python, for the index-build tests.

What it restates (crates/frankensearch-index/src/lib.rs unless said otherwise):
  write_record_with_flags  :3635-3673   dimension, every element finite, usable norm, doc id <= 65,535 bytes
  vector_signal_usable     :6133-6142   norm_sq = one f32 accumulator over the elements in order, separate multiply and add, > 0 and finite
  finish                   :3752-3943   STABLE sort by (FNV-1a(doc id), doc id bytes) :3753-3762, then the FSVI v1 image
  TwoTierIndexBuilder      two_tier.rs:2125-2132   the duplicate rule
and the staging of the device builder: rows are staged encoded, at their arrival position, in chunks of chunk_rows rows; finish reads
staged position perm[i] for slab row i.

FAULTS names the ways an implementation can be wrong that the fixtures must expose: `fault=` puts one of them in place of the
restatement, and tests/test_index_build_contract.py asserts that each changes a verdict or a file byte of the fixtures the GPU test
uses.
"""
import numpy as np

import compaction_ref as CR

FLT_MAX = float(np.finfo(np.float32).max)
FLT_MIN_NORMAL = float(np.finfo(np.float32).tiny)

FAULTS = ("pairwise_norm", "flush_squares", "fma", "unstable_sort", "hash_only_sort", "perm_off_by_chunk", "drop_last_of_chunk",
          "truncate_f16", "clamp_f16")

RULES = {"nonfinite": "all embedding values must be finite",
         "norm": "embedding norm must be non-zero and finite; a zero vector can never match any query",   # lib.rs:3658
         "doc_id_len": "doc_id byte length must fit in u16", "duplicate": "duplicate doc_id; each document must have a unique id"}

# two pairs of distinct strings with one FNV-1a 64 hash each (public knowledge): only the doc id bytes order them
COLLIDING = (("GReLUrM4wMqfg9yzV3KQ", "8yn0iYCKYHlIj4-BwPqk"), ("gMPflVXtwGDXbIhP73TX", "LtHf1prlU1bCeYZEdqWf"))


class Refused(Exception):
    def __init__(self, status, rule=None, row=None):
        super().__init__(f"{status}: {RULES.get(rule, rule)} (row {row})")
        self.status, self.rule, self.row = status, rule, row


# ---- norm_sq and the verdict ------------------------------------------------------------------------------------------------------
def norm_sq_sequential(v):
    """[n, dim] f32 -> [n] f32: the reference's order.  numpy's float32 arithmetic rounds every product and every sum to f32 and keeps
    subnormals."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, np.shape(v)[-1])
    acc = np.zeros(v.shape[0], dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(v.shape[1]):
            p = v[:, j] * v[:, j]
            acc = acc + p
    return acc


def norm_sq_pairwise(v):
    """A pairwise tree over the squares: neighbours are added until one value is left (an odd one is carried up)."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, np.shape(v)[-1])
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        level = v * v
        while level.shape[1] > 1:
            even = level[:, : level.shape[1] // 2 * 2]
            nxt = even[:, 0::2] + even[:, 1::2]
            if level.shape[1] % 2:
                nxt = np.concatenate([nxt, level[:, -1:]], axis=1)
            level = nxt
    return level[:, 0].astype(np.float32)


def norm_sq_flushed(v):
    """Sequential, but a square below the smallest normal f32 is flushed to zero."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, np.shape(v)[-1])
    acc = np.zeros(v.shape[0], dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(v.shape[1]):
            p = v[:, j] * v[:, j]
            p = np.where(np.abs(p) < np.float32(FLT_MIN_NORMAL), np.float32(0), p)
            acc = acc + p
    return acc


def norm_sq_fma(v):
    """Sequential, but acc = fma(x, x, acc): the product is not rounded (f32 x f32 is exact in f64; the sum is rounded once to f64 and
    then to f32, which is the fused result except in double-rounding ties)."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, np.shape(v)[-1])
    acc = np.zeros(v.shape[0], dtype=np.float32)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        for j in range(v.shape[1]):
            x = v[:, j].astype(np.float64)
            acc = (acc.astype(np.float64) + x * x).astype(np.float32)
    return acc


def norm_sq(v, fault=None):
    return {"pairwise_norm": norm_sq_pairwise, "flush_squares": norm_sq_flushed, "fma": norm_sq_fma}.get(fault, norm_sq_sequential)(v)


def row_verdicts(v, fault=None):
    """[n, dim] -> list of None / "nonfinite" / "norm" per row (the finite rule first, as write_record checks it first)."""
    v = np.asarray(v, dtype=np.float32).reshape(-1, np.shape(v)[-1])
    finite = np.all(np.isfinite(v), axis=1)
    ns = norm_sq(v, fault)
    ok = (ns > 0) & np.isfinite(ns)
    return [("nonfinite" if not f else (None if o else "norm")) for f, o in zip(finite, ok)]


# ---- the encodings ----------------------------------------------------------------------------------------------------------------
def encode_rows(v, quant, fault=None):
    """[n, dim] f32 -> [n, dim] of '<f2' (round to nearest even, overflow to +-inf, subnormals kept: f16::from_f32) or '<f4' (as is)."""
    v = np.asarray(v, dtype=np.float32)
    if quant != "f16":
        return v.astype("<f4")
    with np.errstate(over="ignore", under="ignore"):
        h = v.astype("<f2")
    if fault == "truncate_f16":   # round toward zero: one step back wherever rounding went away from zero
        bits = h.view(np.uint16).copy()
        with np.errstate(invalid="ignore"):
            away = np.abs(h.astype(np.float32)) > np.abs(v)
        bits[away] -= 1
        h = bits.view("<f2")
    elif fault == "clamp_f16":    # 65,504 instead of inf
        bits = h.view(np.uint16).copy()
        over = np.isinf(h) & np.isfinite(v)
        bits[over] -= 1
        h = bits.view("<f2")
    return h


# ---- the builder ------------------------------------------------------------------------------------------------------------------
class Builder:
    """add() validates a call as a whole and stages it; finish() is the image and the rows in file order."""

    def __init__(self, dim, quant="f16", embedder_id="test", revision="", gen=0, reject_duplicates=False, chunk_rows=65536, fault=None):
        self.dim, self.quant, self.embedder_id, self.revision, self.gen = dim, quant, embedder_id, revision, gen
        self.reject_duplicates, self.chunk_rows, self.fault = reject_duplicates, chunk_rows, fault
        self.ids = []          # arrival order
        self.staged = []       # position -> row bytes (what the staging chunks hold)
        self.row_bytes = dim * (2 if quant == "f16" else 4)
        self.spent = False

    def record_count(self):
        return len(self.ids)

    def first_refusal(self, doc_ids, v):
        verdicts = row_verdicts(v, self.fault) if len(doc_ids) else []
        seen = set(self.ids) if self.reject_duplicates else None
        for i, d in enumerate(doc_ids):
            if verdicts[i]:
                return verdicts[i], i
            if len(d.encode()) > 0xFFFF:
                return "doc_id_len", i
            if seen is not None:
                if d in seen:
                    return "duplicate", i
                seen.add(d)
        return None

    def add(self, doc_ids, vectors):
        if self.spent:
            raise Refused("InvalidConfig", "spent")
        doc_ids = list(doc_ids)
        v = np.asarray(vectors, dtype=np.float32)
        v = v.reshape(len(doc_ids), -1) if len(doc_ids) else v.reshape(0, self.dim)
        if v.shape[1] != self.dim:
            raise Refused("DimensionMismatch")
        bad = self.first_refusal(doc_ids, v)
        if bad:
            raise Refused("InvalidConfig", bad[0], bad[1])
        enc = encode_rows(v, self.quant, self.fault)
        for i, d in enumerate(doc_ids):
            pos = len(self.ids)
            raw = enc[i].tobytes()
            if self.fault == "drop_last_of_chunk" and pos % self.chunk_rows == self.chunk_rows - 1:
                raw = bytes(self.row_bytes)   # never written: what the fresh chunk held
            self.staged.append(raw)
            self.ids.append(d)

    def order(self):
        n = len(self.ids)
        if self.fault == "unstable_sort":     # equal keys in reverse arrival order
            return sorted(range(n), key=lambda i: CR.sort_key(self.ids[i]) + (-i,))
        if self.fault == "hash_only_sort":
            return sorted(range(n), key=lambda i: CR.sort_key(self.ids[i])[0])
        return sorted(range(n), key=lambda i: CR.sort_key(self.ids[i]))   # sorted() is stable

    def rows(self):
        """(doc id, row bytes) in file order."""
        n = len(self.ids)
        out = []
        for i in self.order():
            src = i
            if self.fault == "perm_off_by_chunk" and i + self.chunk_rows < n:
                src = i + self.chunk_rows
            out.append((self.ids[i], self.staged[src]))
        return out

    def finish(self):
        if self.spent:
            raise Refused("InvalidConfig", "spent")
        self.spent = True
        return CR.fsvi_image(self.rows(), self.dim, self.quant, self.embedder_id, self.revision, self.gen)


# ---- fixtures shared by the contract test and the GPU test ------------------------------------------------------------------------
DIMS = (1, 7, 8, 33, 100, 256, 384, 1024)
NS = (0, 1, 63, 64, 65, 1000, 5000)
CHUNKS = (1, 37, 64, 0)   # 0 = the library default (65,536)
SPLITS = (1, 64, 129)     # rows of the first adds; the rest goes in one more


def cases():
    """56 (dim, n, chunk_rows, quant): every dim with every n, every chunk_rows and both slabs with every dim.  One-row chunks stay with
    the sizes up to 129 rows (5,000 allocations would test the allocator)."""
    out = []
    for i in range(len(DIMS) * len(NS)):
        dim, n = DIMS[i % len(DIMS)], NS[i % len(NS)]
        chunk = CHUNKS[(i + i // len(DIMS)) % len(CHUNKS)]
        if chunk == 1 and n > 129:
            chunk = 37
        quant = "f16" if (i + i // len(DIMS)) % 2 == 0 else "f32"
        out.append((dim, n, chunk, quant))
    return out


SPECIALS = np.array([65504.0, 65520.0, 65519.996, 70000.0, -1.0e9, 1.0e12, 5.9604645e-08, 2.9802322e-08, 2.9802325e-08, 6.0e-08, -6.1e-05,
                     1.0009765625, 1.00048828125, 1.00146484375, -0.0, 0.0, 2049.0, 2051.0, -2049.0, 1.0e-30], dtype=np.float32)
"""Values beyond the f16 range (-> inf; 65,520 is the tie that rounds up to inf, 65,519.996 the last that does not), f16 subnormals and
the halves around the smallest one, ties between neighbouring f16 values (to even: 1.00048828125 -> 1.0, 1.00146484375 -> 1.001953125,
2049 -> 2048, 2051 -> 2052), the zeros, and a value that underflows to zero."""


def fixture(dim, n, seed):
    """n (doc id, vector) in arrival order: random rows salted with SPECIALS, ids with duplicates, the empty id, a 65,535-byte id and the
    colliding pairs (the later-sorting member first) where n has room for them."""
    rng = np.random.default_rng(seed)
    v = rng.standard_normal((n, dim)).astype(np.float32)
    flat = v.reshape(-1)
    if flat.size:
        at = rng.choice(flat.size, size=min(flat.size, max(1, flat.size // 7)), replace=False)
        flat[at] = SPECIALS[rng.integers(0, SPECIALS.size, size=at.size)]
        for r in range(n):   # every row keeps a usable norm whatever the salt did
            if not np.any(np.abs(v[r]) > 1e-3):
                v[r, 0] = 1.0 + r
    ids = [f"doc-{i}" for i in range(n)]
    if n >= 3:
        ids[n // 2] = ids[0]            # a duplicate far apart ...
    if n >= 4:
        ids[n - 1] = ids[n - 2]         # ... and two neighbours
    if n >= 5:
        ids[1] = ""
    if n >= 6:
        ids[3] = "x" * 65535
    if n >= 63:
        (a1, a2), (b1, b2) = COLLIDING
        ids[5], ids[40], ids[7], ids[41] = a1, a2, b1, b2
    return ids, v


def split_adds(n):
    """Ragged adds: 1, 64, 129 rows and then the rest."""
    out, at = [], 0
    for s in SPLITS:
        if at >= n:
            break
        out.append((at, min(n, at + s)))
        at = min(n, at + s)
    if at < n:
        out.append((at, n))
    return out


def boundary_fixture(dim, seed, want=48, batch=2048):
    """Rows whose exact norm_sq lies within 2^-23 (relative) of FLT_MAX, found by a seeded search: random directions scaled to the
    boundary, kept when the f32 row still lies in the window.  Whether such a row's sequential f32 sum is finite depends on the order
    of the additions."""
    rng = np.random.default_rng(seed)
    keep = []
    while sum(len(k) for k in keep) < want:
        v = rng.standard_normal((batch, dim))
        exact = np.sum(v * v, axis=1)
        edge = FLT_MAX * (1.0 + rng.uniform(-1.0, 1.0, size=batch) * 2.0 ** -24)
        c = (v * np.sqrt(edge / exact)[:, None]).astype(np.float32)
        c64 = c.astype(np.float64)
        rel = np.array([abs(float(np.sum(r * r))) for r in c64]) / FLT_MAX - 1.0   # (f64 sums of exact squares: error 2^-50)
        keep.append(c[(np.abs(rel) <= 2.0 ** -23) & np.all(np.isfinite(c), axis=1)])
    return np.concatenate(keep, axis=0)[:want]


def underflow_pair(dim):
    """A row of 1e-23 (every square underflows to zero: refused) and a row of 3e-23 (the squares are f32 subnormals: accepted)."""
    return np.full((1, dim), 1e-23, np.float32), np.full((1, dim), 3e-23, np.float32)

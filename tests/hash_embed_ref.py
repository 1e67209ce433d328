"""CPU restatement of the reference's HashEmbedder (crates/frankensearch-embed/src/hash_embedder.rs), the yardstick of
tests/test_hash_embed_contract.py and tests/test_gpu_hash_embed.py.

  tokenize               :601-685   == text.split(|c| !c.is_alphanumeric()).filter(|t| t.len() >= 2)  (:691-695), len in UTF-8 bytes
  fnv1a_hash             :588-595
  embed_fnv_modular      :263-280
  embed_jl               :299-346   one chain at a time (jl_accumulate_one :339-346), the 8-chain form (:467-481) and the
                                    ballot / popcount form the kernel uses are all here: the contract test holds them equal
  l2_normalize_in_place  crates/frankensearch-core/src/traits.rs:606-618

Pure Python integers for the hashes and the chains, numpy uint64 across tokens for speed, np.float32 for the sequential fold
and the scale.  Which characters are alphanumeric is an argument (a 0x110000-bit table, bit c = byte[c >> 3] >> (c & 7) & 1), as
it is for the library: None means ASCII only."""
import numpy as np

FNV_OFFSET = 0xCBF29CE484222325
FNV_PRIME = 0x100000001B3
MASK = 0xFFFFFFFFFFFFFFFF
MIN_TOKEN_LEN = 2
F32 = np.float32
F32_EPSILON = F32(1.1920929e-7)
BITMAP_BYTES = 0x110000 // 8


def bitmap_from(pred) -> np.ndarray:
    """The table for `pred(chr(c))`."""
    bits = np.fromiter((1 if pred(chr(c)) else 0 for c in range(0x110000)), dtype=np.uint8, count=0x110000)
    return np.packbits(bits, bitorder="little")


_PY_BITMAP = None


def python_bitmap() -> np.ndarray:
    """str.isalnum's table (Python's Unicode tables, not Rust's), computed once and shared."""
    global _PY_BITMAP
    if _PY_BITMAP is None:
        _PY_BITMAP = bitmap_from(str.isalnum)
        _PY_BITMAP.setflags(write=False)
    return _PY_BITMAP


def is_alnum(c: str, bitmap) -> bool:
    o = ord(c)
    if o < 0x80:
        return ("0" <= c <= "9") or ("a" <= c <= "z") or ("A" <= c <= "Z")
    return bitmap is not None and bool((int(bitmap[o >> 3]) >> (o & 7)) & 1)


def tokenize(text: str, bitmap=None):
    """The split rule (:691-695): maximal runs of alphanumeric characters of at least two UTF-8 bytes, as bytes."""
    out, cur = [], []
    for c in text:
        if is_alnum(c, bitmap):
            cur.append(c)
        else:
            if cur:
                out.append("".join(cur).encode())
            cur = []
    if cur:
        out.append("".join(cur).encode())
    return [t for t in out if len(t) >= MIN_TOKEN_LEN]


def fnv1a(b: bytes) -> int:
    h = FNV_OFFSET
    for x in b:
        h = ((h ^ x) * FNV_PRIME) & MASK
    return h


def xorshift(s: int) -> int:
    s ^= (s << 13) & MASK
    s ^= s >> 7
    s ^= (s << 17) & MASK
    return s


def jl_states(hashes, seed: int):
    return [((seed ^ h) | 1) & MASK for h in hashes]


def jl_one_at_a_time(states, dim: int) -> np.ndarray:
    """jl_accumulate_one (:339-346) per token, in f32 as the reference adds."""
    acc = [F32(0.0)] * dim
    for s in states:
        for d in range(dim):
            s = xorshift(s)
            acc[d] = F32(acc[d] + (F32(1.0) if (s & 1) == 0 else F32(-1.0)))
    return np.array(acc, dtype=F32)


def jl_groups_of_8(states, dim: int) -> np.ndarray:
    """embed_jl's own order (:305-322): full groups of JL_LANES = 8 through the 8 - 2 * odd form (:467-481), then the tail one chain
    at a time."""
    acc = [F32(0.0)] * dim
    full = len(states) - len(states) % 8
    for g in range(0, full, 8):
        s = list(states[g:g + 8])
        for d in range(dim):
            odd = 0
            for i in range(8):
                s[i] = xorshift(s[i])
                odd += s[i] & 1
            acc[d] = F32(acc[d] + F32(8 - 2 * odd))
    for s in states[full:]:
        for d in range(dim):
            s = xorshift(s)
            acc[d] = F32(acc[d] + (F32(1.0) if (s & 1) == 0 else F32(-1.0)))
    return np.array(acc, dtype=F32)


def jl_ballot(states, dim: int, width: int = 64) -> np.ndarray:
    """The kernel's formulation: groups of `width` chains, per dimension active - 2 * popcount(odd), in an integer accumulator
    that is converted once.  numpy uint64 across the chains of a group."""
    acc = np.zeros(dim, dtype=np.int64)
    st = np.array(states, dtype=np.uint64)
    for g in range(0, len(st), width):
        s = st[g:g + width].copy()
        active = int(s.size)
        for d in range(dim):
            s ^= s << np.uint64(13)
            s ^= s >> np.uint64(7)
            s ^= s << np.uint64(17)
            acc[d] += active - 2 * int(np.count_nonzero(s & np.uint64(1)))
    return acc.astype(F32)


def jl_accumulate(states, dim: int) -> np.ndarray:
    """All chains at once (what the GPU tests compare against: the three forms above are equal, test_hash_embed_contract)."""
    return jl_ballot(states, dim, width=max(len(states), 1))


def fnv_accumulate(hashes, dim: int) -> np.ndarray:
    acc = np.zeros(dim, dtype=np.int64)
    for h in hashes:
        acc[h % dim] += 1 if (h >> 63) == 1 else -1
    return acc.astype(F32)


def l2_normalize_in_place(v: np.ndarray) -> np.ndarray:
    """traits.rs:606-618: sequential f32 fold of x * x (separate multiply and add), zeros when not finite or < f32::EPSILON."""
    v = np.asarray(v, dtype=F32)
    norm_sq = F32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = v * v   # (each product is one IEEE f32 multiply)
        for x in sq:
            norm_sq = F32(norm_sq + x)
    if not np.isfinite(norm_sq) or norm_sq < F32_EPSILON:
        return np.zeros_like(v)
    inv = F32(F32(1.0) / np.sqrt(norm_sq, dtype=F32))
    return (v * inv).astype(F32)


def embed(text: str, dim: int, algorithm: str = "fnv_modular", seed: int = 0, bitmap=None):
    """HashEmbedder::embed_sync (:245-252) -> (vector f32 [dim], tokens hashed)."""
    hashes = [fnv1a(t) for t in tokenize(text, bitmap)]
    if algorithm == "fnv_modular":
        acc = fnv_accumulate(hashes, dim)
    elif algorithm == "jl":
        acc = jl_accumulate(jl_states(hashes, seed), dim)
    else:
        raise ValueError(algorithm)
    return l2_normalize_in_place(acc), len(hashes)


def jl_accumulate_batch(states_per_text, dim: int) -> np.ndarray:
    """jl_accumulate for many texts in one sweep over the dimensions: every chain of every text advances together (numpy uint64)
    and a text's signs are summed by its segment.  Integer sums, so equal to the per-text forms."""
    n = len(states_per_text)
    acc = np.zeros((n, dim), dtype=np.int64)
    lens = np.array([len(x) for x in states_per_text], dtype=np.int64)
    if lens.sum() == 0:
        return acc.astype(F32)
    s = np.array([x for st in states_per_text for x in st], dtype=np.uint64)
    seg = np.repeat(np.arange(n), lens)
    for d in range(dim):
        s ^= s << np.uint64(13)
        s ^= s >> np.uint64(7)
        s ^= s << np.uint64(17)
        odd = np.bincount(seg, weights=(s & np.uint64(1)).astype(np.float64), minlength=n).astype(np.int64)
        acc[:, d] = lens - 2 * odd
    return acc.astype(F32)


def embed_batch(texts, dim: int, algorithm: str = "fnv_modular", seed: int = 0, bitmap=None, hashes=None):
    """embed for a batch -> (vectors f32 [n, dim], tokens hashed uint32 [n]).  `hashes` (token_hashes(texts, bitmap)) may be passed
    by a caller that embeds the same texts under several configurations."""
    if hashes is None:
        hashes = token_hashes(texts, bitmap)
    if algorithm == "fnv_modular":
        acc = np.stack([fnv_accumulate(h, dim) for h in hashes]) if hashes else np.zeros((0, dim), dtype=F32)
    elif algorithm == "jl":
        acc = jl_accumulate_batch([jl_states(h, seed) for h in hashes], dim)
    else:
        raise ValueError(algorithm)
    out = np.zeros((len(hashes), dim), dtype=F32)
    for i in range(len(hashes)):
        out[i] = l2_normalize_in_place(acc[i])
    return out, np.array([len(h) for h in hashes], dtype=np.uint32)


def token_hashes(texts, bitmap=None):
    return [[fnv1a(t) for t in tokenize(x, bitmap)] for x in texts]

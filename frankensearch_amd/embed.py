"""Embedders — host-side mirror of the reference's SyncEmbed implementations
(crates/frankensearch-core/src/traits.rs:401-582) over libfsgpu.so.  Tokenisation is the caller's
(third-party `tokenizers` in the reference); the boundary is token ids.
"""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence

import numpy as np

from . import _lib
from .errors import check


class Model2VecEmbedder:
    """potion static embedder (crates/frankensearch-embed/src/model2vec_embedder.rs:55-58)."""

    def __init__(self, table: np.ndarray, device: int = 0):
        t = np.ascontiguousarray(table, dtype=np.float32)
        if t.ndim != 2:
            raise TypeError("table must be [vocab, dim] f32")
        self._dim = t.shape[1]
        h = C.c_void_p()
        check(_lib.lib().fsgpu_m2v_create(device, t.ctypes.data, t.shape[0], t.shape[1], C.byref(h)))
        self._h = h

    def dimension(self) -> int:
        return self._dim

    def embed_token_ids(self, ids: Sequence[int]) -> np.ndarray:
        return self.embed_batch_token_ids([ids])[0]

    def embed_batch_token_ids(self, batch: Sequence[Sequence[int]]) -> np.ndarray:
        """embed_batch_sync (model2vec_embedder.rs:409-419) over pre-tokenised texts -> [n, dim] f32."""
        n = len(batch)
        offsets = np.zeros(n + 1, dtype=np.uint32)
        for i, ids in enumerate(batch):
            offsets[i + 1] = offsets[i] + len(ids)
        flat = np.zeros(max(int(offsets[-1]), 1), dtype=np.uint32)
        for i, ids in enumerate(batch):
            flat[offsets[i]:offsets[i + 1]] = np.asarray(ids, dtype=np.uint32)
        return self.embed_flat(flat, offsets)

    def embed_flat(self, ids: np.ndarray, offsets: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """fsgpu_m2v_embed on arrays already in the C ABI's shape: concatenated uint32 ids, uint32 offsets [n + 1]."""
        if ids.dtype != np.uint32 or offsets.dtype != np.uint32 or not ids.flags.c_contiguous or not offsets.flags.c_contiguous:
            raise TypeError("ids and offsets must be contiguous uint32")
        n = offsets.shape[0] - 1
        if out is None:
            out = np.empty((n, self._dim), dtype=np.float32)
        check(_lib.lib().fsgpu_m2v_embed(self._h, ids.ctypes.data, offsets.ctypes.data, n, out.ctypes.data))
        return out

    def set_coalescing(self, max_batch: int, max_wait_us: int = 100) -> None:
        check(_lib.lib().fsgpu_m2v_set_coalescing(self._h, max_batch, max_wait_us))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_m2v_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class _BertConfig(C.Structure):
    _fields_ = [("vocab", C.c_uint32), ("hidden", C.c_uint32), ("layers", C.c_uint32), ("heads", C.c_uint32),
                ("inter", C.c_uint32), ("max_pos", C.c_uint32), ("ln_eps", C.c_float)]


_LAYER_FIELDS = ["q_w", "q_b", "k_w", "k_b", "v_w", "v_b", "ao_w", "ao_b", "ln1_w", "ln1_b", "i_w", "i_b", "o_w", "o_b",
                 "ln2_w", "ln2_b"]


class _BertLayerWeights(C.Structure):
    _fields_ = [(f, C.c_void_p) for f in _LAYER_FIELDS]


class _BertWeights(C.Structure):
    _fields_ = [("word_emb", C.c_void_p), ("pos_emb", C.c_void_p), ("type_emb", C.c_void_p), ("emb_ln_w", C.c_void_p),
                ("emb_ln_b", C.c_void_p), ("layers", C.POINTER(_BertLayerWeights))]


_HF_LAYER_KEYS = {
    "q_w": "attention.self.query.weight", "q_b": "attention.self.query.bias",
    "k_w": "attention.self.key.weight", "k_b": "attention.self.key.bias",
    "v_w": "attention.self.value.weight", "v_b": "attention.self.value.bias",
    "ao_w": "attention.output.dense.weight", "ao_b": "attention.output.dense.bias",
    "ln1_w": "attention.output.LayerNorm.weight", "ln1_b": "attention.output.LayerNorm.bias",
    "i_w": "intermediate.dense.weight", "i_b": "intermediate.dense.bias",
    "o_w": "output.dense.weight", "o_b": "output.dense.bias",
    "ln2_w": "output.LayerNorm.weight", "ln2_b": "output.LayerNorm.bias",
}


class _BertOptions(C.Structure):
    _fields_ = [("linear_format", C.c_uint32), ("reserved", C.c_uint32 * 7)]


# fsgpu_bert_options.linear_format (include/fsgpu.h): the keyword of NativeEmbedder -> FSGPU_BERT_LINEAR_*
LINEAR_FORMATS = {"f16": 0, "int8_dynamic": 1}


def _bert_options(linear: str):
    """None for "f16" (the library's default, through the original create calls); an fsgpu_bert_options otherwise."""
    if linear not in LINEAR_FORMATS:
        raise ValueError(f"linear must be one of {sorted(LINEAR_FORMATS)}, not {linear!r}")
    return None if linear == "f16" else _BertOptions(LINEAR_FORMATS[linear])


class NativeEmbedder:
    """MiniLM-class BERT embedder (crates/frankensearch-rerank/src/native_embedder.rs:40-50).

    `weights` is a dict of f32 arrays in the HuggingFace key layout; bare `embeddings.*` / `encoder.*` keys are
    normalised to the `bert.` prefix exactly like `parse_weights` (native.rs:1466-1476).

    `linear` chooses the arithmetic of the linears at create time: "f16" (the default: f16 matrix-core linears) or
    "int8_dynamic" (the reference's native forward: int8 per-output-channel weights, per-row dynamic int8 activations; within
    cosine 0.995 / max-abs 6e-2 of the f32 forward instead of 0.999 / 2e-3, and bitwise the same vector for a text whatever
    batch it rides in — DESIGN §3.8)."""

    def __init__(self, weights: dict, device: int = 0, ln_eps: float = 1e-12, linear: str = "f16"):
        opts = _bert_options(linear)
        w = {}
        for k, v in weights.items():
            if k.startswith("embeddings.") or k.startswith("encoder."):
                k = "bert." + k
            w[k] = np.ascontiguousarray(v, dtype=np.float32)
        word = w["bert.embeddings.word_embeddings.weight"]
        pos = w["bert.embeddings.position_embeddings.weight"]
        layers = 0
        while f"bert.encoder.layer.{layers}.attention.self.query.weight" in w:
            layers += 1
        hidden = word.shape[1]
        inter = w["bert.encoder.layer.0.intermediate.dense.weight"].shape[0]
        cfg = _BertConfig(word.shape[0], hidden, layers, hidden // 32, inter, min(pos.shape[0], 512), ln_eps)
        lw = (_BertLayerWeights * layers)()
        for i in range(layers):
            for f, key in _HF_LAYER_KEYS.items():
                setattr(lw[i], f, w[f"bert.encoder.layer.{i}.{key}"].ctypes.data)
        bw = _BertWeights(word.ctypes.data, pos.ctypes.data,
                          w["bert.embeddings.token_type_embeddings.weight"].ctypes.data,
                          w["bert.embeddings.LayerNorm.weight"].ctypes.data,
                          w["bert.embeddings.LayerNorm.bias"].ctypes.data, lw)
        self._dim = hidden
        h = C.c_void_p()
        if opts is None:
            check(_lib.lib().fsgpu_bert_create(device, C.byref(cfg), C.byref(bw), C.byref(h)))
        else:
            check(_lib.lib().fsgpu_bert_create_ex(device, C.byref(cfg), C.byref(bw), C.byref(opts), C.byref(h)))
        self._h = h

    @classmethod
    def from_safetensors(cls, path: str, device: int = 0, ln_eps: float = 1e-12, linear: str = "f16") -> "NativeEmbedder":
        """NativeEmbedder::load (native_embedder.rs:60-116): the model file goes to the library as it is — the safetensors header and
        the HuggingFace key layout are parsed behind the C ABI (fsgpu_bert_create_safetensors = parse_weights, native.rs:1359-1602)."""
        with open(path, "rb") as f:
            return cls.from_safetensors_bytes(f.read(), device=device, ln_eps=ln_eps, linear=linear)

    @classmethod
    def from_safetensors_bytes(cls, blob: bytes, device: int = 0, ln_eps: float = 1e-12, linear: str = "f16") -> "NativeEmbedder":
        opts = _bert_options(linear)
        buf = np.frombuffer(blob, dtype=np.uint8)   # (numpy's buffer of a bytes object is 16-byte aligned past its header: checked by the library)
        if buf.ctypes.data % 8:
            buf = np.require(buf.copy(), requirements=["ALIGNED"])
        self = cls.__new__(cls)
        h = C.c_void_p()
        if opts is None:
            check(_lib.lib().fsgpu_bert_create_safetensors(device, buf.ctypes.data, buf.size, ln_eps, C.byref(h)))
        else:
            check(_lib.lib().fsgpu_bert_create_safetensors_ex(device, buf.ctypes.data, buf.size, ln_eps, C.byref(opts), C.byref(h)))
        self._h = h
        self._dim = int(_lib.lib().fsgpu_bert_dimension(h))
        return self

    def dimension(self) -> int:
        return self._dim

    @property
    def linear_format(self) -> str:
        """The `linear` keyword this embedder was created with ("f16" or "int8_dynamic"), as the library reports it."""
        code = int(_lib.lib().fsgpu_bert_linear_format(self._h))
        return {v: k for k, v in LINEAR_FORMATS.items()}[code]

    def embed_token_ids(self, ids: Sequence[int]) -> np.ndarray:
        return self.embed_batch_token_ids([ids])[0]

    def embed_batch_token_ids(self, batch: Sequence[Sequence[int]]) -> np.ndarray:
        """embed_batch_sync (native_embedder.rs:218-255) over pre-tokenised texts (special tokens included)."""
        n = len(batch)
        offsets = np.zeros(n + 1, dtype=np.uint32)
        for i, ids in enumerate(batch):
            offsets[i + 1] = offsets[i] + len(ids)
        flat = np.zeros(max(int(offsets[-1]), 1), dtype=np.int32)
        for i, ids in enumerate(batch):
            flat[offsets[i]:offsets[i + 1]] = np.asarray(ids, dtype=np.int32)
        return self.embed_flat(flat, offsets)

    def embed_flat(self, ids: np.ndarray, offsets: np.ndarray, out: np.ndarray = None) -> np.ndarray:
        """The C ABI as a host holds it after tokenisation (fsgpu_bert_embed): concatenated int32 ids, uint32 offsets
        [n + 1]; text i owns ids[offsets[i]:offsets[i + 1]].  No per-text Python work (the list marshalling of
        embed_batch_token_ids costs ~0.3 ms per 256 texts, more than half the GPU forward)."""
        if ids.dtype != np.int32 or offsets.dtype != np.uint32 or not ids.flags.c_contiguous or not offsets.flags.c_contiguous:
            raise TypeError("ids must be contiguous int32 and offsets contiguous uint32")
        n = offsets.shape[0] - 1
        if out is None:
            out = np.empty((n, self._dim), dtype=np.float32)
        check(_lib.lib().fsgpu_bert_embed(self._h, ids.ctypes.data, offsets.ctypes.data, n, out.ctypes.data))
        return out

    def set_coalescing(self, max_batch: int, max_wait_us: int = 200) -> None:
        check(_lib.lib().fsgpu_bert_set_coalescing(self._h, max_batch, max_wait_us))

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_bert_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# fsgpu_hash_create's algorithm (include/fsgpu.h): the keyword of HashEmbedder -> FSGPU_HASH_*
HASH_ALGORITHMS = {"fnv_modular": 0, "jl": 1}
ALNUM_BITMAP_BYTES = 0x110000 // 8


def python_alnum_bitmap() -> np.ndarray:
    """The alphanumeric table of fsgpu_hash_create (0x110000 bits, bit c = byte[c >> 3] >> (c & 7) & 1) built from `str.isalnum`.

    These are PYTHON's tables, not Rust's: `char::is_alphanumeric` is Alphabetic | Nd | Nl | No of the Rust toolchain's Unicode
    version, `str.isalnum` is the L* | Nd | Nl | No categories of this interpreter's, and the two differ on the `Other_Alphabetic`
    combining marks (and wherever the Unicode versions differ).  A host that wants the reference's bits passes the table its own
    toolchain gives."""
    bits = np.zeros(0x110000, dtype=np.uint8)
    for c in range(0x110000):
        if chr(c).isalnum():
            bits[c] = 1
    return np.packbits(bits, bitorder="little")


def _text_arrays(texts: Sequence[str]):
    """Texts -> the C ABI's shape: UTF-8 bytes back to back (uint8) and uint32 offsets [n + 1]."""
    raw = [t if isinstance(t, (bytes, bytearray)) else str(t).encode("utf-8", "surrogatepass") for t in texts]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint32)
    total = 0
    for i, b in enumerate(raw):
        total += len(b)
        if total > 0xFFFFFFFF:
            raise ValueError("a batch of texts must stay below 4 GiB")
        offsets[i + 1] = total
    flat = np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8)
    return flat, offsets


class HashEmbedder:
    """The hash embedder (crates/frankensearch-embed/src/hash_embedder.rs:201-328): raw text in, no weights.  `algorithm` is
    "fnv_modular" (HashAlgorithm::FnvModular) or "jl" (JLProjection { seed }).  `alnum_bitmap` (139,264 bytes, see
    python_alnum_bitmap) says which code points above U+007F are alphanumeric; without one the embedder is ASCII only and refuses
    any other text.  A refused text raises with `.bad_text` set to its index in the call; nothing is written."""

    def __init__(self, dimension: int = 384, algorithm: str = "fnv_modular", seed: int = 0, device: int = 0, alnum_bitmap=None):
        if isinstance(algorithm, str):
            if algorithm not in HASH_ALGORITHMS:
                raise ValueError(f"algorithm must be one of {sorted(HASH_ALGORITHMS)}, not {algorithm!r}")
            algorithm = HASH_ALGORITHMS[algorithm]
        bm = None
        if alnum_bitmap is not None:
            bm = np.ascontiguousarray(alnum_bitmap, dtype=np.uint8).reshape(-1)
            if bm.size != ALNUM_BITMAP_BYTES:
                raise ValueError(f"alnum_bitmap must hold {ALNUM_BITMAP_BYTES} bytes")
        h = C.c_void_p()
        check(_lib.lib().fsgpu_hash_create(device, dimension, algorithm, seed & 0xFFFFFFFFFFFFFFFF, None if bm is None else bm.ctypes.data,
                                           C.byref(h)))
        self._h = h
        self._dim = dimension
        self.device = device
        self.last_token_counts = None

    @classmethod
    def default_384(cls, **kw) -> "HashEmbedder":
        return cls(384, "fnv_modular", **kw)

    @classmethod
    def default_256(cls, **kw) -> "HashEmbedder":
        return cls(256, "fnv_modular", **kw)

    @classmethod
    def jl_384(cls, seed: int, **kw) -> "HashEmbedder":
        return cls(384, "jl", seed, **kw)

    def dimension(self) -> int:
        return self._dim

    def _call(self, fn, texts, out_ptr):
        from .errors import SearchError
        flat, offsets = _text_arrays(texts)
        n = offsets.shape[0] - 1
        counts = np.zeros(n, dtype=np.uint32)
        bad = C.c_uint32(0xFFFFFFFF)
        try:
            check(fn(self._h, flat.ctypes.data, offsets.ctypes.data, n, out_ptr, counts.ctypes.data, C.byref(bad)))
        except SearchError as e:
            e.bad_text = None if bad.value == 0xFFFFFFFF else int(bad.value)
            raise
        self.last_token_counts = counts

    def embed(self, texts: Sequence[str], out: np.ndarray = None) -> np.ndarray:
        """embed_batch_sync (hash_embedder.rs:254-260) -> [n, dimension] f32; `last_token_counts` holds the tokens hashed per text."""
        if out is None:
            out = np.empty((len(texts), self._dim), dtype=np.float32)
        self._call(_lib.lib().fsgpu_hash_embed, texts, out.ctypes.data)
        return out

    def embed_device(self, texts: Sequence[str], out_ptr: int) -> None:
        """... into [n, dimension] f32 of the embedder's device (a torch tensor's data_ptr(), fsgpu_device_malloc)."""
        self._call(_lib.lib().fsgpu_hash_embed_device, texts, out_ptr)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_hash_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

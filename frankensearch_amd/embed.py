"""Embedders — host-side mirror of the reference's SyncEmbed implementations
(crates/frankensearch-core/src/traits.rs:401-582) over libfsgpu.so.  The encoders' boundary is token ids;
WordPieceTokenizer makes them on the device from raw text (the reference uses third-party `tokenizers`), and
Model2VecEmbedder.embed_texts takes text straight through.
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

    def embed_texts(self, tokenizer: "WordPieceTokenizer", texts: Sequence[str], out: np.ndarray = None) -> np.ndarray:
        """embed_batch_sync from raw text (model2vec_embedder.rs:280-335): tokenised on the device without special tokens or
        truncation (encode_fast(text, false)), the ids never leave it.  A text the device tokenizer leaves to the host raises with
        `.bad_text` set to its index; nothing is written."""
        flat, offsets = _text_arrays(texts)
        n = offsets.shape[0] - 1
        if out is None:
            out = np.empty((n, self._dim), dtype=np.float32)
        _call_with_bad_text(_lib.lib().fsgpu_m2v_embed_texts, self._h, tokenizer._h, flat.ctypes.data, offsets.ctypes.data, n,
                            out.ctypes.data)
        return out

    def embed_texts_device(self, tokenizer: "WordPieceTokenizer", texts: Sequence[str], out_ptr: int) -> None:
        """... into [n, dim] f32 of the embedder's device."""
        flat, offsets = _text_arrays(texts)
        _call_with_bad_text(_lib.lib().fsgpu_m2v_embed_texts_device, self._h, tokenizer._h, flat.ctypes.data, offsets.ctypes.data,
                            offsets.shape[0] - 1, out_ptr)

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

    def embed_texts(self, tokenizer: "WordPieceTokenizer", texts: Sequence[str], max_length=None, out: np.ndarray = None) -> np.ndarray:
        """embed_batch_sync from raw text (native_embedder.rs:172-255): `[CLS] pieces [SEP]`, truncated to `max_length` (None: the
        tokenizer file's truncation, 0: none), tokenised on the device; the forward reads the ids where they lie and gives the
        bits embed_flat gives for the same ids.  A text the device tokenizer leaves to the host raises with `.bad_text` set to its
        index; nothing is written."""
        flat, offsets = _text_arrays(texts)
        n = offsets.shape[0] - 1
        if out is None:
            out = np.empty((n, self._dim), dtype=np.float32)
        _call_with_bad_text(_lib.lib().fsgpu_bert_embed_texts, self._h, tokenizer._h, flat.ctypes.data, offsets.ctypes.data, n,
                            tokenizer.max_length if max_length is None else int(max_length), out.ctypes.data)
        return out

    def embed_texts_device(self, tokenizer: "WordPieceTokenizer", texts: Sequence[str], out_ptr: int, max_length=None) -> None:
        """... into [n, hidden] f32 of the embedder's device."""
        flat, offsets = _text_arrays(texts)
        _call_with_bad_text(_lib.lib().fsgpu_bert_embed_texts_device, self._h, tokenizer._h, flat.ctypes.data, offsets.ctypes.data,
                            offsets.shape[0] - 1, tokenizer.max_length if max_length is None else int(max_length), out_ptr)

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


def _call_with_bad_text(fn, *args):
    """A C call whose last argument is out_bad_text: a refusal raises with `.bad_text` = the text's index in the call, or None."""
    from .errors import SearchError
    bad = C.c_uint32(0xFFFFFFFF)
    try:
        check(fn(*args, C.byref(bad)))
    except SearchError as e:
        e.bad_text = None if bad.value == 0xFFFFFFFF else int(bad.value)
        raise


# fsgpu_wordpiece_config.cp_info (include/fsgpu.h)
WP_CODE_POINTS = 0x110000
WP_VALUE_MASK = 0x1FFFFF
WP_LEN_SHIFT = 21
WP_SPACE = 1 << 24
WP_ISOLATE = 1 << 25
WP_HOST = 1 << 26

_CP_TABLES = {}


def bert_codepoint_table(lowercase: bool = True, strip_accents=None, handle_chinese_chars: bool = True, clean_text: bool = True):
    """(cp_info uint32[0x110000], expansions uint32[...]) of fsgpu_wordpiece_create, made by driving `tokenizers`' own
    BertNormalizer and BertPreTokenizer once per code point, so the table carries whatever Unicode data that library was built
    with.  The only place `tokenizers` is needed; a few seconds, cached per option set.

    An entry is the normalizer's output for the code point alone.  ' X ' (the padding of handle_chinese_chars) is X as a word on
    its own.  HOST: an output of more than 3 code points, an output of 2..3 that holds a separator or a word on its own, and any
    surviving code point with a non-zero combining class (NFD may reorder it against its neighbours, which no per-code-point
    table can express)."""
    key = (bool(lowercase), strip_accents, bool(handle_chinese_chars), bool(clean_text))
    if key in _CP_TABLES:
        return _CP_TABLES[key]
    import unicodedata
    from tokenizers.normalizers import BertNormalizer
    from tokenizers.pre_tokenizers import BertPreTokenizer
    norm = BertNormalizer(clean_text=clean_text, handle_chinese_chars=handle_chinese_chars, strip_accents=strip_accents,
                          lowercase=lowercase)
    pre = BertPreTokenizer()
    outs = [""] * WP_CODE_POINTS
    for c in range(WP_CODE_POINTS):
        if not 0xD800 <= c <= 0xDFFF:   # (no text holds a surrogate)
            outs[c] = norm.normalize_str(chr(c))
    # the class of every normalised code point, from the pre-tokenizer itself: "x?x" stays whole, splits in two or in three
    alphabet = sorted(set("".join(outs)))
    klass = {}
    for base in range(0, len(alphabet), 4096):
        chunk = alphabet[base:base + 4096]
        toks = [t for t, _ in pre.pre_tokenize_str(" ".join("x" + o + "x" for o in chunk))]
        at = 0
        for o in chunk:
            if toks[at] == "x" + o + "x":
                klass[o], at = 0, at + 1
            elif toks[at] == "x" and toks[at + 1] == o and toks[at + 2] == "x":
                klass[o], at = WP_ISOLATE, at + 3
            elif toks[at] == "x" and toks[at + 1] == "x":
                klass[o], at = WP_SPACE, at + 2
            else:
                raise RuntimeError(f"BertPreTokenizer treats U+{ord(o):04X} in a way the table cannot express")
        if at != len(toks):
            raise RuntimeError("BertPreTokenizer's pieces do not add up")
    info = np.zeros(WP_CODE_POINTS, dtype=np.uint32)
    expansions = []
    memo = {}
    for c in range(WP_CODE_POINTS):
        out = outs[c]
        if not out:
            continue
        entry = memo.get(out) if len(out) == 1 else None
        if entry is None:
            isolate = 0
            o = out
            if len(o) == 3 and o[0] == " " and o[2] == " " and klass[o[1]] != WP_SPACE:
                o, isolate = o[1], WP_ISOLATE
            if len(o) > 3 or any(unicodedata.combining(x) for x in o) or (len(o) > 1 and any(klass[x] for x in o)):
                entry = WP_HOST
            elif len(o) == 1:
                entry = ord(o) | (1 << WP_LEN_SHIFT) | klass[o] | isolate
                if entry & WP_SPACE:
                    entry &= ~WP_ISOLATE
            else:
                entry = len(expansions) | (len(o) << WP_LEN_SHIFT)
                expansions.extend(ord(x) for x in o)
            if len(out) == 1:
                memo[out] = entry
        info[c] = entry
    table = (info, np.asarray(expansions or [0], dtype=np.uint32)[:len(expansions)].copy())
    _CP_TABLES[key] = table
    return table


class _WordPieceConfig(C.Structure):
    _fields_ = [("vocab_bytes", C.c_void_p), ("vocab_offsets", C.c_void_p), ("vocab_size", C.c_uint32), ("unk_id", C.c_uint32),
                ("cls_id", C.c_uint32), ("sep_id", C.c_uint32), ("prefix_bytes", C.c_void_p), ("prefix_len", C.c_uint32),
                ("max_input_chars_per_word", C.c_uint32), ("cp_info", C.c_void_p), ("expansions", C.c_void_p),
                ("expansions_len", C.c_uint32), ("added_bytes", C.c_void_p), ("added_offsets", C.c_void_p),
                ("added_count", C.c_uint32), ("reserved", C.c_uint32 * 8)]


def _blob(items):
    """Byte strings -> (uint8 blob, uint32 offsets [len + 1]) of the C ABI."""
    raw = [x if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8") for x in items]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint32)
    if raw:
        offsets[1:] = np.cumsum([len(b) for b in raw], dtype=np.uint64).astype(np.uint32)
    return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), offsets


class WordPieceTokenizer:
    """The BERT WordPiece tokenizer on the device (fsgpu_wordpiece_*): BertNormalizer -> BertPreTokenizer ->
    WordPiece -> [CLS] ... [SEP], ids equal to `tokenizers`' for the same tokenizer.json.  `vocab` is the tokens in id order;
    `cp_info` / `expansions` are the per-code-point table (bert_codepoint_table); `added` the added tokens' contents.  A text
    that holds an added token's content or a code point the table marks HOST is flagged (status 1, no ids): it is the host
    tokenizer's.  Padding, offsets, word ids and token strings are not produced."""

    def __init__(self, vocab, unk_id: int, cls_id: int, sep_id: int, cp_info, expansions, added=(), prefix="##",
                 max_input_chars_per_word: int = 100, device: int = 0, max_length: int = 0, reserved=None):
        self.vocab_bytes, self.vocab_offsets = _blob(vocab)
        self.added_bytes, self.added_offsets = _blob(added)
        self.prefix = prefix if isinstance(prefix, (bytes, bytearray)) else str(prefix).encode("utf-8")
        self.cp_info = np.ascontiguousarray(cp_info, dtype=np.uint32).reshape(-1)
        if self.cp_info.size != WP_CODE_POINTS:
            raise ValueError(f"cp_info must hold {WP_CODE_POINTS} entries")
        self.expansions = np.ascontiguousarray(expansions, dtype=np.uint32).reshape(-1)
        self.unk_id, self.cls_id, self.sep_id = int(unk_id), int(cls_id), int(sep_id)
        self.max_input_chars_per_word = int(max_input_chars_per_word)
        self.max_length = int(max_length)   # the file's truncation, the default of encode / encode_pairs (0: none)
        self.device = device
        prefix_arr = np.frombuffer(self.prefix or b"\0", dtype=np.uint8).copy()
        cfg = _WordPieceConfig(self.vocab_bytes.ctypes.data, self.vocab_offsets.ctypes.data, len(self.vocab_offsets) - 1, self.unk_id,
                               self.cls_id, self.sep_id, prefix_arr.ctypes.data, len(self.prefix), self.max_input_chars_per_word,
                               self.cp_info.ctypes.data, self.expansions.ctypes.data if self.expansions.size else None,
                               self.expansions.size, self.added_bytes.ctypes.data, self.added_offsets.ctypes.data,
                               len(self.added_offsets) - 1)
        for i, r in enumerate(reserved or ()):
            cfg.reserved[i] = r
        h = C.c_void_p()
        check(_lib.lib().fsgpu_wordpiece_create(device, C.byref(cfg), C.byref(h)))
        self._h = h

    @staticmethod
    def parse_tokenizer_json(path_or_str) -> dict:
        """The keyword arguments of the constructor (without the code-point table, whose options come back under "normalizer")
        from a tokenizer.json, read with the `json` module.  Anything but BertNormalizer -> BertPreTokenizer -> WordPiece ->
        [CLS] A [SEP] / [CLS] A [SEP] B [SEP], truncated longest_first from the right without stride, is refused."""
        import json
        import os
        text = path_or_str
        if isinstance(text, (bytes, bytearray)):
            text = text.decode("utf-8")
        if not text.lstrip().startswith("{"):
            with open(os.fspath(path_or_str), encoding="utf-8") as f:
                text = f.read()
        doc = json.loads(text)

        def refuse(why):
            raise ValueError(f"tokenizer.json is not the BERT WordPiece pipeline the device tokenizer serves: {why}")

        model = doc.get("model") or {}
        kind = model.get("type") or ("BPE" if "merges" in model else "WordPiece" if "continuing_subword_prefix" in model else "?")
        if kind != "WordPiece":
            refuse(f"model type {kind}")
        norm = doc.get("normalizer") or {}
        if norm.get("type") != "BertNormalizer":
            refuse(f"normalizer {norm.get('type')}")
        if (doc.get("pre_tokenizer") or {}).get("type") != "BertPreTokenizer":
            refuse(f"pre-tokenizer {(doc.get('pre_tokenizer') or {}).get('type')}")
        trunc = doc.get("truncation")
        max_length = 0
        if trunc:
            squash = lambda s: str(s).replace("_", "").lower()
            if squash(trunc.get("strategy", "LongestFirst")) != "longestfirst":
                refuse(f"truncation strategy {trunc.get('strategy')}")
            if squash(trunc.get("direction", "Right")) != "right":
                refuse(f"truncation direction {trunc.get('direction')}")
            if trunc.get("stride", 0) != 0:
                refuse(f"truncation stride {trunc.get('stride')}")
            max_length = int(trunc["max_length"])
        vocab_map = model.get("vocab") or {}
        vocab = [None] * len(vocab_map)
        for tok, i in vocab_map.items():
            if not 0 <= i < len(vocab) or vocab[i] is not None:
                refuse("the vocabulary's ids are not 0..n-1")
            vocab[i] = tok
        unk = model.get("unk_token", "[UNK]")
        if unk not in vocab_map:
            refuse(f"the unknown token {unk!r} is not in the vocabulary")
        post = doc.get("post_processor")
        if post is None:
            cls_tok, sep_tok = "[CLS]", "[SEP]"
        elif post.get("type") == "BertProcessing":
            cls_tok, sep_tok = post["cls"][0], post["sep"][0]
        elif post.get("type") == "TemplateProcessing":
            shape = lambda seq: [("S", p["SpecialToken"]["id"], p["SpecialToken"]["type_id"]) if "SpecialToken" in p
                                 else ("Q", p["Sequence"]["id"], p["Sequence"]["type_id"]) for p in seq]
            single, pair = shape(post.get("single", [])), shape(post.get("pair", []))
            if len(single) != 3 or [k for k, _, _ in single] != ["S", "Q", "S"] or [t for _, _, t in single] != [0, 0, 0]:
                refuse("the single-sequence template is not [CLS] $A [SEP]")
            cls_tok, sep_tok = single[0][1], single[2][1]
            if pair != [("S", cls_tok, 0), ("Q", "A", 0), ("S", sep_tok, 0), ("Q", "B", 1), ("S", sep_tok, 1)]:
                refuse("the pair template is not [CLS] $A [SEP] $B:1 [SEP]:1")
            for tok in (cls_tok, sep_tok):
                if post["special_tokens"][tok]["ids"] != [vocab_map.get(tok)]:
                    refuse(f"the template's {tok} is not the vocabulary's")
        else:
            refuse(f"post-processor {post.get('type')}")
        for tok in (cls_tok, sep_tok):
            if tok not in vocab_map:
                refuse(f"{tok!r} is not in the vocabulary")
        added = []
        for a in doc.get("added_tokens") or []:
            if a.get("normalized"):
                refuse(f"added token {a.get('content')!r} is matched against normalised text")
            added.append(a["content"])
        return {"vocab": vocab, "unk_id": vocab_map[unk], "cls_id": vocab_map[cls_tok], "sep_id": vocab_map[sep_tok], "added": added,
                "prefix": model.get("continuing_subword_prefix", "##"),
                "max_input_chars_per_word": int(model.get("max_input_chars_per_word", 100)), "max_length": max_length,
                "normalizer": {"lowercase": norm.get("lowercase", True), "strip_accents": norm.get("strip_accents"),
                               "handle_chinese_chars": norm.get("handle_chinese_chars", True),
                               "clean_text": norm.get("clean_text", True)}}

    @classmethod
    def from_tokenizer_json(cls, path_or_str, device: int = 0, table=None) -> "WordPieceTokenizer":
        """From a tokenizer.json (a path or the text itself).  `table` = (cp_info, expansions); without one it is built from
        `tokenizers` with the file's normalizer options (bert_codepoint_table)."""
        kw = cls.parse_tokenizer_json(path_or_str)
        options = kw.pop("normalizer")
        cp_info, expansions = table if table is not None else bert_codepoint_table(**options)
        return cls(cp_info=cp_info, expansions=expansions, device=device, **kw)

    def vocab_size(self) -> int:
        return int(_lib.lib().fsgpu_wordpiece_vocab_size(self._h))

    def _length(self, max_length):
        return self.max_length if max_length is None else int(max_length)

    def encode_flat(self, flat: np.ndarray, offsets: np.ndarray, add_special_tokens: bool = True, max_length=None, capacity=None):
        """fsgpu_wordpiece_encode on arrays in the C ABI's shape -> (ids uint32, offsets uint32 [n + 1], status uint8 [n]).
        `capacity` (ids the output may hold) defaults to a bound no text can pass: its bytes plus the two special tokens."""
        n = offsets.shape[0] - 1
        if capacity is None:
            capacity = int(offsets[-1]) - int(offsets[0]) + 2 * n if n else 0
        ids = np.zeros(max(capacity, 1), dtype=np.uint32)
        out_offsets = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(n, dtype=np.uint8)
        total = C.c_uint64(0)
        self.last_total = None
        try:
            _call_with_bad_text(_lib.lib().fsgpu_wordpiece_encode, self._h, flat.ctypes.data, offsets.ctypes.data, n,
                                1 if add_special_tokens else 0, self._length(max_length), ids.ctypes.data, capacity,
                                out_offsets.ctypes.data, status.ctypes.data, C.byref(total))
        finally:
            self.last_total = int(total.value)
        return ids[:total.value], out_offsets, status

    def encode(self, texts: Sequence[str], add_special_tokens: bool = True, max_length=None):
        """Tokenizer.encode_batch(texts).ids as a CSR: (ids, offsets [n + 1], status [n]); status 1 = left to the host, no ids."""
        flat, offsets = _text_arrays(texts)
        return self.encode_flat(flat, offsets, add_special_tokens, max_length)

    def encode_device(self, texts: Sequence[str], ids_ptr: int, capacity: int, offsets_ptr: int, add_special_tokens: bool = True,
                      max_length=None):
        """... with ids [capacity] and offsets [n + 1] (uint32) left in memory of the tokenizer's device -> (status, total)."""
        flat, offsets = _text_arrays(texts)
        n = offsets.shape[0] - 1
        status = np.zeros(n, dtype=np.uint8)
        total = C.c_uint64(0)
        _call_with_bad_text(_lib.lib().fsgpu_wordpiece_encode_device, self._h, flat.ctypes.data, offsets.ctypes.data, n,
                            1 if add_special_tokens else 0, self._length(max_length), ids_ptr, capacity, offsets_ptr,
                            status.ctypes.data, C.byref(total))
        return status, int(total.value)

    def encode_pairs(self, a_texts: Sequence[str], b_texts: Sequence[str], max_length=None, capacity=None):
        """Tokenizer.encode_batch(list(zip(a, b))) -> (ids, type_ids, offsets [n + 1], status [n]): [CLS] a [SEP] b [SEP]."""
        if len(a_texts) != len(b_texts):
            raise ValueError("a_texts and b_texts must pair up")
        a_flat, a_off = _text_arrays(a_texts)
        b_flat, b_off = _text_arrays(b_texts)
        n = a_off.shape[0] - 1
        if capacity is None:
            capacity = int(a_off[-1]) + int(b_off[-1]) + 3 * n
        ids = np.zeros(max(capacity, 1), dtype=np.uint32)
        types = np.zeros(max(capacity, 1), dtype=np.uint32)
        out_offsets = np.zeros(n + 1, dtype=np.uint32)
        status = np.zeros(n, dtype=np.uint8)
        total = C.c_uint64(0)
        self.last_total = None
        try:
            _call_with_bad_text(_lib.lib().fsgpu_wordpiece_encode_pairs, self._h, a_flat.ctypes.data, a_off.ctypes.data,
                                b_flat.ctypes.data, b_off.ctypes.data, n, self._length(max_length), ids.ctypes.data, types.ctypes.data,
                                capacity, out_offsets.ctypes.data, status.ctypes.data, C.byref(total))
        finally:
            self.last_total = int(total.value)
        return ids[:total.value], types[:total.value], out_offsets, status

    def encode_pairs_device(self, a_texts: Sequence[str], b_texts: Sequence[str], ids_ptr: int, type_ids_ptr: int, capacity: int,
                            offsets_ptr: int, max_length=None):
        a_flat, a_off = _text_arrays(a_texts)
        b_flat, b_off = _text_arrays(b_texts)
        n = a_off.shape[0] - 1
        status = np.zeros(n, dtype=np.uint8)
        total = C.c_uint64(0)
        _call_with_bad_text(_lib.lib().fsgpu_wordpiece_encode_pairs_device, self._h, a_flat.ctypes.data, a_off.ctypes.data,
                            b_flat.ctypes.data, b_off.ctypes.data, n, self._length(max_length), ids_ptr, type_ids_ptr, capacity,
                            offsets_ptr, status.ctypes.data, C.byref(total))
        return status, int(total.value)

    def close(self) -> None:
        if getattr(self, "_h", None) is not None and self._h.value:
            _lib.lib().fsgpu_wordpiece_destroy(self._h)
            self._h = C.c_void_p(None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

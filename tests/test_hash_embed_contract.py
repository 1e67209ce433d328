"""The hash embedder without a GPU: tests/hash_embed_ref.py (the yardstick of test_gpu_hash_embed.py) is held to the reference's own
literals (crates/frankensearch-embed/src/hash_embedder.rs, test module :687-998), and the library judges a configuration before
it looks for a device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hash_embed_ref as R  # noqa: E402

F32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def table(alnum_above_ascii: str) -> np.ndarray:
    """An explicit table: exactly these characters above U+007F are alphanumeric."""
    bm = np.zeros(R.BITMAP_BYTES, dtype=np.uint8)
    for c in alnum_above_ascii:
        bm[ord(c) >> 3] |= 1 << (ord(c) & 7)
    return bm


def split_rule(text: str, bitmap):
    """text.split(|c| !c.is_alphanumeric()).filter(|t| t.len() >= 2) (:691-695), stated on its own: separators become one
    character that no token holds."""
    marked = "".join(c if R.is_alnum(c, bitmap) else "\n" for c in text)
    return [t.encode() for t in marked.split("\n") if len(t.encode()) >= 2]


def test_fnv1a_literals():
    assert R.fnv1a(b"") == 0xCBF29CE484222325   # fnv1a_empty_is_offset_basis :983
    assert R.fnv1a(b"a") == 0xAF63DC4C8601EC8C   # the published FNV-1a 64 vectors
    assert R.fnv1a(b"foobar") == 0x85944171F73967E8


def test_tokenize_lists_of_the_reference():
    bm = table("éΔ京")
    assert R.tokenize("hello world", bm) == [b"hello", b"world"]                                   # :950-953
    assert R.tokenize("a bb ccc", bm) == [b"bb", b"ccc"]                                           # :956-959
    assert R.tokenize("a é Δ 京", bm) == ["é".encode(), "Δ".encode(), "京".encode()]               # :962-965: len is UTF-8 bytes
    assert R.tokenize("hello-world.test", bm) == [b"hello", b"world", b"test"]                     # :968-971
    assert R.tokenize("Hello WORLD", bm) == [b"Hello", b"WORLD"]                                   # :974-978: case preserved
    assert R.tokenize("a é Δ 京", None) == []   # without a table nothing above U+007F is alphanumeric


def test_tokenize_matches_the_split_rule_on_the_five_strings():
    # tokenizer_matches_unicode_split_reference :699-705
    bm = table("\u00e9\u00efΔ日本語")   # U+0301 clear: the combining mark ends the first token
    want = {
        "": [],
        "a an ant, fox_42 jumps-over C3PO": [b"an", b"ant", b"fox", b"42", b"jumps", b"over", b"C3PO"],
        "snake_case HTTP/2 path/to/file.rs": [b"snake", b"case", b"HTTP", b"path", b"to", b"file", b"rs"],
        "cafe\u0301 caf\u00e9 na\u00efve 日本語 x": [b"cafe", "caf\u00e9".encode(), "na\u00efve".encode(), "日本語".encode()],
        "a.b::c -- Δelta42": ["Δelta42".encode()],
    }
    for text, tokens in want.items():
        assert R.tokenize(text, bm) == tokens, text
        assert split_rule(text, bm) == tokens, text
    marks = table("\u00e9\u00efΔ日本語\u0301")   # ... and with U+0301 set it joins it
    assert R.tokenize("cafe\u0301 x", marks) == split_rule("cafe\u0301 x", marks) == ["cafe\u0301".encode()]
    py = R.python_bitmap()
    for text in want:
        assert R.tokenize(text, py) == split_rule(text, py), text


def norm_f32(v):
    s = F32(0)
    for x in v * v:
        s = F32(s + x)
    return float(np.sqrt(s, dtype=F32))


@pytest.mark.parametrize("algorithm,seed", [("fnv_modular", 0), ("jl", 42)])
def test_vectors_of_the_reference(algorithm, seed):
    for text in ("", "a b c"):   # empty_string_produces_zero_vector, single_char_tokens_filtered :921-935
        v, count = R.embed(text, 384, algorithm, seed)
        assert count == 0 and v.shape == (384,) and np.all(bits(v) == 0)
    v, count = R.embed("hello world", 384, algorithm, seed)   # output_is_l2_normalized :893-909
    assert count == 2 and abs(norm_f32(v) - 1.0) < 1e-6
    v, count = R.embed("word " * 20000, 384, algorithm, seed)
    assert count == 20000 and v.shape == (384,)
    if algorithm == "fnv_modular":   # long_input_no_panic :938-945 (default_384, as there); every token lands in one bucket
        assert abs(norm_f32(v) - 1.0) < 1e-6
        h = R.fnv1a(b"word")
        want = np.zeros(384, dtype=F32)
        want[h % 384] = 1.0 if h >> 63 else -1.0
        assert np.array_equal(bits(v), bits(want))


def test_the_long_text_is_past_exact_f32_sums():
    # the sequential fold is observable: 20,000 tokens put the sum of squares past 2^24, where the order of the adds decides bits
    acc = R.jl_accumulate(R.jl_states([R.fnv1a(b"word")] * 20000, 42), 384)
    assert float((acc.astype(np.float64) ** 2).sum()) > 2.0 ** 24


@pytest.mark.parametrize("count", [0, 1, 7, 8, 9, 63, 64, 65, 200])
def test_jl_formulations_agree_bit_for_bit(count):
    # jl_ilp_matches_scalar_across_token_counts :846-859, plus the wave-wide ballot / popcount form of the kernel
    text = " ".join("tok%03d" % i for i in range(count))
    states = R.jl_states([R.fnv1a(t) for t in R.tokenize(text)], 7)
    assert len(states) == count
    one = R.jl_one_at_a_time(states, 384)
    assert np.array_equal(bits(one), bits(R.jl_groups_of_8(states, 384)))
    assert np.array_equal(bits(one), bits(R.jl_ballot(states, 384, 64)))
    assert np.array_equal(bits(one), bits(R.jl_accumulate(states, 384)))
    assert np.array_equal(bits(one), bits(R.jl_accumulate_batch([[], states, states[:5]], 384)[1]))
    v, n = R.embed(text, 384, "jl", 7)
    assert n == count and np.array_equal(bits(v), bits(R.l2_normalize_in_place(one)))


def test_seed_equal_to_a_hash_keeps_the_chain_alive():
    h = R.fnv1a(b"hello")
    assert R.jl_states([h], h) == [1]   # seed ^ hash == 0: the `| 1` rule (:310-313)
    v, _ = R.embed("hello", 64, "jl", h)
    assert abs(norm_f32(v) - 1.0) < 1e-6


def test_configuration_is_judged_before_a_device_is_needed():
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd.build import build

    build()
    for dimension, algorithm in ((0, 0), (1025, 0), (0, 1), (1025, 1), (384, 7), (384, -1)):
        with pytest.raises(fa.InvalidConfig) as err:
            fa.HashEmbedder(dimension, algorithm)
        assert str(err.value)
    with pytest.raises(ValueError):
        fa.HashEmbedder(384, "md5")
    with pytest.raises(ValueError):
        fa.HashEmbedder(384, alnum_bitmap=np.zeros(16, np.uint8))
    if not torch.cuda.is_available():
        for make in (fa.HashEmbedder.default_384, fa.HashEmbedder.default_256, lambda: fa.HashEmbedder.jl_384(42),
                     lambda: fa.HashEmbedder(1024, "jl", alnum_bitmap=R.python_bitmap()), lambda: fa.HashEmbedder(1)):
            with pytest.raises(fa.NoDevice):
                make()


def test_python_alnum_bitmap_is_str_isalnum():
    import frankensearch_amd as fa
    bm = fa.python_alnum_bitmap()
    assert bm.dtype == np.uint8 and bm.size == 139264
    assert np.array_equal(bm, R.python_bitmap())
    for c in "aZ09é京Δ":
        assert (bm[ord(c) >> 3] >> (ord(c) & 7)) & 1
    for c in " _-\u0301":
        assert not (bm[ord(c) >> 3] >> (ord(c) & 7)) & 1

"""GPU checks of the hash embedder (hash_embed_kernels.hip, hash_embedder.cpp) through the Python mirror of the C ABI.  Every
comparison is on f32 BITS, plus the token counts, against tests/hash_embed_ref.py (held to the reference's literals by
test_hash_embed_contract.py).  The texts are built once and their token hashes shared by every case; the alphanumeric table is
Python's (str.isalnum) on both sides: the table is the caller's data, the kernel's job is to follow it."""
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import hash_embed_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
STRIDE = 256     # bytes a workgroup classifies per step (hash_embed_kernels.hip kThreads)
CHUNK = 1024     # states of the JL kernel's LDS list (kHashEmbedChunkStates); it is flushed once more than CHUNK - STRIDE are held
SEED_OF_HELLO = R.fnv1a(b"hello")   # seed ^ hash == 0 for the token "hello": the `| 1` rule
SEEDS = [0, 42, 2 ** 64 - 1, SEED_OF_HELLO]
DIMS = [1, 2, 7, 63, 64, 65, 256, 384, 1024]


def _fa():
    from frankensearch_amd.build import build
    build()
    import frankensearch_amd as fa
    return fa


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def words(n, start=0):
    return " ".join("w%dx" % (start + i) for i in range(n))


def _texts():
    t = {}
    for n in (0, 1, 63, 64, 65, 127, 128, 129):            # around one and two waves of chains
        t["count-%d" % n] = words(n)
    t["count-flush-1"] = words(CHUNK - STRIDE + 200, 1000)   # one flush inside the loop, the rest at the end
    t["count-flush-3"] = words(3 * CHUNK + 17, 5000)        # several flushes: beyond a single LDS chunk
    t["hello"] = "hello"                                    # begins with a token and ends inside it
    t["begins-with-token"] = "alpha, beta"
    t["ends-inside-token"] = "-- alpha beta"
    t["one-byte-alnum"] = "a"
    t["one-byte-other"] = "-"
    t["only-separators"] = " .,;\n\t--"
    t["single-chars"] = "a b c"
    # a token ends at the last byte of one text and the next begins with a token: they must not merge across the offset
    t["adjacent-1"] = "xy ab"
    t["adjacent-2"] = "cd zw"
    t["adjacent-3"] = "q z"      # ... nor may two 1-byte tokens merge into a 2-byte one
    t["adjacent-4"] = "z q"
    # a token straddling the byte stride, ending exactly at it, and beginning exactly at it
    t["straddle-token"] = "-" * (STRIDE - 3) + "abcdefgh tail"
    t["token-ends-at-stride"] = "-" * (STRIDE - 4) + "abcd" + " next"
    t["token-begins-at-stride"] = "-" * STRIDE + "abcd"
    for name, ch in (("2", "é"), ("3", "京"), ("4", "\U0001d518")):   # 2-, 3- and 4-byte alphanumerics
        assert ch.isalnum() and len(ch.encode()) == int(name)
        t["char-%s-alone" % name] = ch
        t["char-%s-words" % name] = "a %s%s b%s %s" % (ch, ch, ch, ch)
        for back in range(1, int(name)):   # the character straddles the stride with `back` of its bytes before it
            t["char-%s-straddle-%d" % (name, back)] = "-" * (STRIDE - back) + ch + "z after"
            t["char-%s-prev-straddle-%d" % (name, back)] = "x" * (STRIDE - back) + ch + "z after"
    t["emoji-separates"] = "ab\U0001f600cd \U0001f600 e\U0001f600f"   # a 4-byte non-alphanumeric
    t["combining-mark"] = "cafe\u0301 caf\u00e9 na\u00efve 日本語 x"   # U+0301 is clear in the table: "cafe" ends at it
    t["reference-case-2"] = "a an ant, fox_42 jumps-over C3PO"
    t["reference-case-5"] = "a.b::c -- Δelta42"
    t["conformance-1"] = "Frankensearch identity"     # HASH_CONFORMANCE_TEXTS_V1 :46-51
    t["conformance-2"] = "Case CASE case"
    t["conformance-3"] = "unicode café 東京"
    t["token-10000-bytes"] = "pre " + "x" * 10000 + " post"
    t["token-10000-bytes-multibyte"] = "é" * 5000
    # multi-byte characters and tokens across every stride and across the flushes of the state list
    t["unicode-long"] = " ".join("日本%d語é" % i for i in range(CHUNK + 300))
    return t


_CACHE = {}


def shared():
    """The texts, their token hashes under Python's table (computed once) and the table."""
    if not _CACHE:
        t = _texts()
        bm = R.python_bitmap()
        assert not (bm[0x0301 >> 3] >> (0x0301 & 7)) & 1
        texts = list(t.values())
        _CACHE.update(names=list(t.keys()), texts=texts, bitmap=bm, hashes=R.token_hashes(texts, bm))
    return _CACHE


def test_the_texts_cover_what_they_claim():
    s = shared()
    counts = dict(zip(s["names"], (len(h) for h in s["hashes"])))
    for n in (0, 1, 63, 64, 65, 127, 128, 129):
        assert counts["count-%d" % n] == n
    assert CHUNK - STRIDE < counts["count-flush-1"] <= CHUNK and counts["count-flush-3"] > 3 * CHUNK and counts["unicode-long"] > CHUNK
    assert counts["one-byte-alnum"] == counts["one-byte-other"] == counts["single-chars"] == counts["adjacent-3"] == 0
    assert counts["char-2-alone"] == counts["char-3-alone"] == counts["char-4-alone"] == 1
    assert counts["emoji-separates"] == 2 and counts["combining-mark"] == 4 and counts["token-10000-bytes"] == 3
    assert SEED_OF_HELLO in s["hashes"][s["names"].index("hello")]


@pytest.mark.parametrize("dim", DIMS)
@pytest.mark.parametrize("algorithm", ["fnv_modular", "jl"])
def test_bits_and_token_counts(algorithm, dim):
    fa = _fa()
    s = shared()
    for seed in (SEEDS if algorithm == "jl" else [0]):
        e = fa.HashEmbedder(dim, algorithm, seed, alnum_bitmap=s["bitmap"])
        assert e.dimension() == dim
        got = e.embed(s["texts"])
        counts = e.last_token_counts.copy()
        e.close()
        want, want_counts = R.embed_batch(s["texts"], dim, algorithm, seed, hashes=s["hashes"])
        assert np.array_equal(counts, want_counts), [n for n, a, b in zip(s["names"], counts, want_counts) if a != b]
        bad = [n for n, a, b in zip(s["names"], bits(got), bits(want)) if not np.array_equal(a, b)]
        assert bad == [], (seed, bad)


@pytest.mark.parametrize("algorithm", ["fnv_modular", "jl"])
def test_exact_fold_of_the_long_text(algorithm):
    """"word " x 20,000 at dim 384 (long_input_no_panic :938-945): the squares sum past 2^24, so the sequential order of the fold
    decides bits."""
    fa = _fa()
    text = "word " * 20000
    e = fa.HashEmbedder(384, algorithm, 42)   # ASCII: no table needed
    got = e.embed([text])[0]
    assert e.last_token_counts.tolist() == [20000]
    want, n = R.embed(text, 384, algorithm, 42)
    assert n == 20000 and np.array_equal(bits(got), bits(want))
    if algorithm == "fnv_modular":   # every token lands in one bucket, +-20,000 before the scale
        h = R.fnv1a(b"word")
        one = np.zeros(384, dtype=F32)
        one[h % 384] = 1.0 if h >> 63 else -1.0
        assert np.array_equal(bits(got), bits(one))
    else:
        acc = R.jl_accumulate(R.jl_states([R.fnv1a(b"word")] * 20000, 42), 384)
        assert float((acc.astype(np.float64) ** 2).sum()) > 2.0 ** 24
    e.close()


ILL_FORMED = {
    "overlong-2": b"ab \xc0\xaf cd", "overlong-3": b"ab \xe0\x80\xaf cd", "overlong-4": b"ab \xf0\x80\x80\xaf cd",
    "surrogate": b"ab \xed\xa0\x80 cd", "past-10ffff": b"ab \xf4\x90\x80\x80 cd", "f5": b"ab \xf5\x80\x80\x80 cd",
    "stray-continuation": b"ab \x80 cd", "truncated-2": b"ab \xc3", "truncated-3": b"ab \xe4\xba", "truncated-4": b"ab \xf0\x9d\x94",
    "cut-by-next-lead": b"ab \xe4\xba\xc3\xa9",
}


def test_refusals_name_the_text_and_write_nothing():
    fa = _fa()
    ascii_only = fa.HashEmbedder(64, "jl", 1)
    out = np.full((3, 64), 7.0, dtype=F32)
    with pytest.raises(fa.InvalidConfig, match="0x80") as err:
        ascii_only.embed(["plain", "café", "naïve"], out=out)
    assert err.value.bad_text == 1 and np.all(out == 7.0)
    assert np.array_equal(bits(ascii_only.embed(["plain"])), bits(R.embed_batch(["plain"], 64, "jl", 1)[0]))   # the handle still serves
    with_table = fa.HashEmbedder(64, "fnv_modular", alnum_bitmap=shared()["bitmap"])
    for why, raw in ILL_FORMED.items():
        for at in (0, 2):
            batch = [b"good one", "café".encode(), b"fine"]
            batch.insert(at, raw)
            out = np.full((4, 64), 7.0, dtype=F32)
            with pytest.raises(fa.InvalidConfig, match="UTF-8") as err:
                with_table.embed(batch, out=out)
            assert err.value.bad_text == at and np.all(out == 7.0), why
    # a text past 32 MiB could hold 2^24 tokens, where the exact-integer argument ends: refused before anything is copied
    out = np.full((2, 64), 7.0, dtype=F32)
    with pytest.raises(fa.InvalidConfig, match="32 MiB") as err:
        with_table.embed([b"ok", b"a" * ((32 << 20) + 1)], out=out)
    assert err.value.bad_text == 1 and np.all(out == 7.0)
    ascii_only.close()
    with_table.close()


@pytest.mark.parametrize("algorithm", ["fnv_modular", "jl"])
def test_a_text_has_the_same_bits_wherever_it_rides(algorithm):
    import torch
    fa = _fa()
    s = shared()
    e = fa.HashEmbedder(384, algorithm, 42, alnum_bitmap=s["bitmap"])
    probe = "The quick brown fox, café 東京 42 times"
    want, n_tok = R.embed(probe, 384, algorithm, 42, s["bitmap"])
    alone = e.embed([probe])
    assert np.array_equal(bits(alone[0]), bits(want)) and e.last_token_counts.tolist() == [n_tok]
    filler = [words(3 + i % 50, i) for i in range(256)]
    for at in (0, 128, 256):   # first, in the middle and last of a 257-text batch
        batch = filler[:at] + [probe] + filler[at:]
        got = e.embed(batch)
        assert got.shape == (257, 384) and np.array_equal(bits(got[at]), bits(want)), at
        assert int(e.last_token_counts[at]) == n_tok
    # a short text after a long one on the same handle: nothing of the long one's workspace shows
    e.embed([s["texts"][s["names"].index(name)] for name in ("count-flush-3", "unicode-long")])
    assert np.array_equal(bits(e.embed(["ab"])[0]), bits(R.embed("ab", 384, algorithm, 42)[0]))
    assert np.array_equal(bits(e.embed([probe])), bits(alone))
    assert np.all(bits(e.embed([""])) == 0) and e.last_token_counts.tolist() == [0]
    assert e.embed([]).shape == (0, 384)
    # embed == embed_device
    batch = filler[:40] + [probe, "", "a b c"]
    host = e.embed(batch)
    host_counts = e.last_token_counts.copy()
    dev = torch.full((len(batch), 384), 7.0, dtype=torch.float32, device="cuda:0")
    e.embed_device(batch, dev.data_ptr())
    assert np.array_equal(bits(dev.cpu().numpy()), bits(host)) and np.array_equal(e.last_token_counts, host_counts)
    assert np.all(bits(host[-2:]) == 0)
    e.close()


def _docs(n):
    rng = np.random.default_rng(5)
    vocab = ["w%d" % i for i in range(300)] + ["alpha", "beta", "gamma", "delta", "HTTP", "C3PO", "x9"]
    return [" ".join(vocab[j] for j in rng.integers(0, len(vocab), 3 + i % 9)) + (". " if i % 2 else "") for i in range(n)]


@pytest.mark.parametrize("algorithm,dim", [("fnv_modular", 384), ("jl", 256)])
def test_raw_text_to_index_end_to_end(tmp_path, oracle, algorithm, dim):
    """2,000 short ASCII documents through IndexBuilder.add_texts(HashEmbedder): the file equals the one IndexBuilder.add writes from
    the restatement's vectors, and a hash-embedded query finds the oracle's rows with the oracle's score bits."""
    fa = _fa()
    n = 2000
    docs = _docs(n)
    ids = ["doc-%04d" % i for i in range(n)]
    e = fa.HashEmbedder(dim, algorithm, 9)
    via_texts = fa.IndexBuilder(dim, "hash", "r1", chunk_rows=512)
    for lo, hi in ((0, 700), (700, 701), (701, n)):
        via_texts.add_texts(e, ids[lo:hi], docs[lo:hi])
    assert via_texts.record_count() == n
    p_texts, p_vectors = str(tmp_path / "texts.fsvi"), str(tmp_path / "vectors.fsvi")
    idx = via_texts.finish(p_texts)
    want, _ = R.embed_batch(docs, dim, algorithm, 9)
    via_vectors = fa.IndexBuilder(dim, "hash", "r1", chunk_rows=512)
    via_vectors.add(ids, want)
    via_vectors.finish(p_vectors).close()
    image = open(p_texts, "rb").read()
    assert image == open(p_vectors, "rb").read()
    slab = np.frombuffer(image[len(image) - n * dim * 2:], dtype="<u2").reshape(n, dim)
    queries = ["alpha beta", docs[17], "w7 w8 w9 gamma", "nothing-here zzz"]
    qv = e.embed(queries)
    assert np.array_equal(bits(qv), bits(R.embed_batch(queries, dim, algorithm, 9)[0]))
    for q in qv:
        hits = idx.search_top_k(q, 10)
        rows, scores = oracle.search_top_k(slab, q, 10)
        assert [h.index for h in hits] == rows.tolist()
        assert np.array_equal(bits([h.score for h in hits]), bits(scores))
    # an empty (and a token-less) document embeds to zeros: refused by the builder's norm rule, naming its row; nothing staged
    b = fa.IndexBuilder(dim, "hash", "r1")
    for batch, row in ((["ab cd", "ef", ""], 2), (["ab cd", "a b c", "ef"], 1)):
        with pytest.raises(fa.InvalidConfig, match="embedding norm must be non-zero and finite") as err:
            b.add_texts(e, ["a", "b", "c"], batch)
        assert err.value.bad_row == row and b.record_count() == 0
    with pytest.raises(fa.InvalidConfig, match="0x80") as err:   # a text the embedder refuses is the call's bad row
        b.add_texts(e, ["a", "b"], ["fine", "café"])
    assert err.value.bad_row == 1 and b.record_count() == 0
    with pytest.raises(fa.DimensionMismatch):
        fa.IndexBuilder(dim + 8, "hash", "r1").add_texts(e, ["a"], ["ab"])
    idx.close()
    e.close()


def test_rust_hash_vectors_golden():
    """tests/golden/rust_hash_vectors.json, when a maintainer has produced it: {"alnum_above_ascii": [code points of
    the texts' non-ASCII characters that char::is_alphanumeric accepts], "vectors": [{"text", "dimension", "algorithm", "seed",
    "bits": [u32]}]} over HASH_CONFORMANCE_TEXTS_V1 (:46-51).  Absent here (no Rust toolchain): skipped."""
    path = os.path.join(os.path.dirname(__file__), "golden", "rust_hash_vectors.json")
    if not os.path.exists(path):
        pytest.skip("tests/golden/rust_hash_vectors.json not provided (see INTEGRATION.md)")
    fa = _fa()
    gold = json.load(open(path))
    bm = np.zeros(R.BITMAP_BYTES, dtype=np.uint8)
    for c in gold["alnum_above_ascii"]:
        bm[c >> 3] |= 1 << (c & 7)
    for v in gold["vectors"]:
        e = fa.HashEmbedder(v["dimension"], v["algorithm"], int(v["seed"]), alnum_bitmap=bm)
        got = bits(e.embed([v["text"]])[0]).tolist()
        e.close()
        assert got == [int(b) for b in v["bits"]], v["text"]
        assert got == bits(R.embed(v["text"], v["dimension"], v["algorithm"], int(v["seed"]), bm)[0]).tolist()

"""GPU checks of the device WordPiece tokenizer (wordpiece_kernels.hip, wordpiece.cpp) through the Python mirror of the C ABI.
Ids, offsets and statuses must EQUAL those of tests/wordpiece_ref.py (held to `tokenizers` by test_wordpiece_contract.py), and
`tokenizers`' own where it imports.  The code-point table, the vocabularies, the texts and the restatement's answers are built
once and shared."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import wordpiece_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
STRIDE = 256     # bytes a workgroup decodes per step (wordpiece_kernels.hip kThreads)
WINDOW = 2048    # normalised code points of the LDS window (kCap)
SENTINEL = 0xDEADBEEF

_STATE = {}


def rows(ids, offsets):
    return [list(map(int, ids[offsets[i]:offsets[i + 1]])) for i in range(len(offsets) - 1)]


def filler(nbytes):
    """Exactly nbytes bytes of short ASCII words."""
    return ("ab cd efg " * (nbytes // 10 + 1))[:nbytes]


def _texts():
    t = {}
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        t["bytes-%d" % n] = filler(n)
    t["longer-than-the-window"] = filler(3 * WINDOW + 77)
    t["one-word-longer-than-the-window"] = "x" * (WINDOW + 900) + " ab"
    t["long-words-across-windows"] = filler(WINDOW - 40) + "q" * 100 + " " + filler(WINDOW - 90) + "z" * 101 + " ab " + "w" * 1500 + " cd"
    t["punctuation-fills-the-window"] = "," * (WINDOW + 300)
    # 2-, 3- and 4-byte characters straddling the byte step, one byte at a time
    for name, ch in (("2", "ß"), ("3", "中"), ("4", "\U0001f600")):
        for back in range(1, len(ch.encode())):
            t["straddle-%s-%d" % (name, back)] = filler(STRIDE - back - 1) + " " + ch + "ab " + ch
    for n in (99, 100, 101):
        t["word-%d-ascii" % n] = "ab " + "x" * n + " cd"
        t["word-%d-two-byte" % n] = "ß" * n
        t["word-%d-accents" % n] = "é" * n + " ö"           # 2 bytes in, 1 code point out
        t["word-%d-mixed" % n] = ("aß\U00010428д" * 26)[:n]    # 1-, 2-, 4- and 2-byte characters (U+10428 is in the vocabulary)
        t["word-%d-hangul" % n] = "각" * (n // 3) + "ᄀ" * (n % 3)   # counted in normalised code points: 3 per syllable
    t["two-pieces-then-fails"] = "ab\U0001f9ff cd"
    t["hangul-opens"] = "각 한글"
    t["dropped-characters-join"] = "a​b a\u0000b a�b"
    t["cjk-inside-a-word"] = "ab中cd"
    t["only-separators"] = "  \t\n 　 "
    t["adjacent-1"] = "ab"
    t["adjacent-2"] = "cd"
    t["adjacent-3"] = "ef "
    t["case-and-accents"] = "Hello, Wörld! İSTANBUL ǅ ﬁ ẞ Σίσυφος"
    t["unknown-letters"] = "ab ŧŧ cd"
    t["punctuation-runs"] = "a.b,c!!d--e [x] {y}"
    for k in (5, 6, 7):
        t["pieces-%d" % k] = " ".join("a" for _ in range(k))
    return t


def state():
    if not _STATE:
        from frankensearch_amd.build import build
        build()
        import frankensearch_amd as fa
        from frankensearch_amd.embed import WordPieceTokenizer, bert_codepoint_table
        cp_info, expansions = bert_codepoint_table()
        vocab = R.synthetic_vocab()
        text = R.tokenizer_json(vocab)
        kw = WordPieceTokenizer.parse_tokenizer_json(text)
        kw.pop("normalizer")
        texts = _texts()
        names = list(texts)
        ref = R.WordPieceRef(cp_info=cp_info, expansions=expansions, **kw)
        try:
            from tokenizers import Tokenizer
            hf = Tokenizer.from_str(text)
        except ImportError:
            hf = None
        _STATE.update(fa=fa, cp_info=cp_info, expansions=expansions, vocab=vocab, json=text, kw=kw, ref=ref, hf=hf, names=names,
                      texts=[texts[k] for k in names], tok=WordPieceTokenizer.from_tokenizer_json(text, table=(cp_info, expansions)))
        _STATE["want"] = {sp: ref.encode(_STATE["texts"], add_special_tokens=sp, max_length=0) for sp in (True, False)}
    return _STATE


def same_csr(got, want):
    assert np.array_equal(got[1], want[1]), "offsets"
    assert np.array_equal(got[0], want[0]), "ids"
    assert np.array_equal(got[2], want[2]), "statuses"


def test_ids_offsets_and_statuses_equal_the_restatement():
    s = state()
    for special in (True, False):
        got = s["tok"].encode(s["texts"], add_special_tokens=special, max_length=0)
        want = s["want"][special]
        got_rows, want_rows = rows(got[0], got[1]), rows(want[0], want[1])
        for name, g, w in zip(s["names"], got_rows, want_rows):
            assert g == w, name
        same_csr(got, want)
        assert not got[2].any()
        if s["hf"] is not None:
            assert got_rows == [e.ids for e in s["hf"].encode_batch(s["texts"], add_special_tokens=special)]
    # what the cases are there for
    want = dict(zip(s["names"], rows(*s["want"][False][:2])))
    unk = s["kw"]["unk_id"]
    assert unk not in want["word-100-ascii"] and want["word-101-ascii"].count(unk) == 1
    assert unk not in want["word-100-two-byte"] and want["word-101-two-byte"] == [unk]
    assert unk not in want["word-99-hangul"] and want["word-101-hangul"] == [unk]
    assert want["two-pieces-then-fails"][0] == unk and want["two-pieces-then-fails"][1:] == want["adjacent-2"]
    assert want["one-word-longer-than-the-window"][0] == unk and want["one-word-longer-than-the-window"][1:] == want["adjacent-1"]
    assert want["only-separators"] == [] and len(want["punctuation-fills-the-window"]) == WINDOW + 300


def test_a_real_size_vocabulary():
    s = state()
    from frankensearch_amd.embed import WordPieceTokenizer
    vocab = R.random_vocab()
    assert len(vocab) == 30522
    text = R.tokenizer_json(vocab)
    kw = WordPieceTokenizer.parse_tokenizer_json(text)
    kw.pop("normalizer")
    ref = R.WordPieceRef(cp_info=s["cp_info"], expansions=s["expansions"], **kw)
    tok = WordPieceTokenizer.from_tokenizer_json(text, table=(s["cp_info"], s["expansions"]))
    rng = np.random.default_rng(5)
    alphabet = np.asarray(list(R.LETTERS) + list("0123456789") + R.JAMO[:8] + list("ßдα") + [" "] * 8 + list(".,中"), dtype=object)
    texts = ["".join(rng.choice(alphabet, size=int(rng.integers(0, 200)))) for _ in range(300)]
    got, want = tok.encode(texts), ref.encode(texts, max_length=0)
    same_csr(got, want)
    if s["hf"] is not None:
        from tokenizers import Tokenizer
        assert rows(got[0], got[1]) == [e.ids for e in Tokenizer.from_str(text).encode_batch(texts)]
    unk = kw["unk_id"]
    share = float(np.mean(got[0] == unk))
    assert 0.0 < share < 0.9, share   # both hits and misses were exercised
    tok.close()


def test_truncation_of_single_sequences():
    s = state()
    texts = [" ".join("a" for _ in range(k)) for k in (0, 1, 5, 6, 7, 8, 300)]
    for special in (True, False):
        for max_length in (2, 8):
            # (max_length 8 with special tokens: the texts of 5, 6 and 7 pieces are at max_length - 1, max_length and max_length + 1)
            got = s["tok"].encode(texts, add_special_tokens=special, max_length=max_length)
            same_csr(got, s["ref"].encode(texts, add_special_tokens=special, max_length=max_length))
            assert max(np.diff(got[1].astype(np.int64))) == max_length
    with pytest.raises(s["fa"].InvalidConfig):
        s["tok"].encode(texts, add_special_tokens=True, max_length=1)


def test_pairs_on_the_grid():
    s = state()
    sizes = range(0, 14)
    a_texts = [" ".join("a" for _ in range(a)) for a in sizes for _ in sizes]
    b_texts = [" ".join("b" for _ in range(b)) for _ in sizes for b in sizes]
    for max_length in (0, 8, 9):
        got = s["tok"].encode_pairs(a_texts, b_texts, max_length=max_length)
        want = s["ref"].encode_pairs(a_texts, b_texts, max_length=max_length)
        for g, w, what in zip(got, want, ("ids", "type ids", "offsets", "statuses")):
            assert np.array_equal(g, w), (what, max_length)
    # pairs of real texts, one of them flagged
    a_texts = ["what is ab?", "ab [SEP] cd", "", "Hello"]
    b_texts = [s["texts"][s["names"].index("longer-than-the-window")], "fine", "cd", ""]
    got = s["tok"].encode_pairs(a_texts, b_texts, max_length=64)
    want = s["ref"].encode_pairs(a_texts, b_texts, max_length=64)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    assert list(got[3]) == [0, 1, 0, 0]
    with pytest.raises(s["fa"].InvalidConfig):
        s["tok"].encode_pairs(["a"], ["b"], max_length=2)


def test_a_flagged_text_between_two_good_ones():
    s = state()
    # (a spacing mark with a non-zero combining class survives strip_accents, which removes Mn only)
    host = next(chr(c) for c in (0x302E, 0x302F, 0x1D165, 0x1D16D) if int(s["cp_info"][c]) & R.WP_HOST)
    texts = ["good one", "ab [SEP] cd", "fine", "ab" + host + "cd", "x [MASK]", filler(700) + "[CLS]", "[sep] [ CLS ]"]
    got = s["tok"].encode(texts)
    same_csr(got, s["ref"].encode(texts, max_length=0))
    assert list(got[2]) == [0, 1, 0, 1, 1, 1, 0]
    assert got[1][2] == got[1][1] and got[1][4] == got[1][3]


def raw_encode(tok, data: bytes, offsets, capacity, special=1, max_length=0):
    from frankensearch_amd import _lib
    flat = np.frombuffer(data or b"\0", dtype=np.uint8).copy()
    offsets = np.asarray(offsets, dtype=np.uint32)
    n = len(offsets) - 1
    ids = np.full(max(capacity, 1), SENTINEL, dtype=np.uint32)
    out_offsets = np.full(n + 1, SENTINEL, dtype=np.uint32)
    status = np.full(max(n, 1), 0xEE, dtype=np.uint8)
    total, bad = C.c_uint64(SENTINEL), C.c_uint32(SENTINEL)
    rc = _lib.lib().fsgpu_wordpiece_encode(tok._h, flat.ctypes.data, offsets.ctypes.data, n, special, max_length, ids.ctypes.data,
                                           capacity, out_offsets.ctypes.data, status.ctypes.data, C.byref(total), C.byref(bad))
    return rc, ids, out_offsets, status, total.value, bad.value


def test_refusals_write_nothing():
    s = state()
    tok = s["tok"]
    untouched = lambda ids, offs, status: (ids == SENTINEL).all() and (offs == SENTINEL).all() and (status == 0xEE).all()
    for why, bad in {"truncated": b"ab \xe4\xb8", "overlong": b"\xc0\xaf", "surrogate": b"\xed\xa0\x80", "stray": b"a\x80b",
                     "past U+10FFFF": b"\xf4\x90\x80\x80"}.items():
        data = b"good" + bad + b"fine"
        rc, ids, offs, status, total, bad_text = raw_encode(tok, data, [0, 4, 4 + len(bad), len(data)], 64)
        assert rc == 2 and bad_text == 1, why
        assert untouched(ids, offs, status), why
    rc, ids, offs, status, total, bad_text = raw_encode(tok, b"abcdefgh", [0, 6, 4, 8], 64)
    assert rc == 2 and untouched(ids, offs, status)
    # too small an ids_capacity: the total is reported, nothing else is written
    want = s["ref"].encode(["ab cd", " ef"], max_length=0)
    need = len(want[0])
    rc, ids, offs, status, total, bad_text = raw_encode(tok, b"ab cd ef", [0, 5, 8], need - 1)
    assert rc == 2 and total == need and bad_text == 0xFFFFFFFF and untouched(ids, offs, status)
    rc, ids, offs, status, total, bad_text = raw_encode(tok, b"ab cd ef", [0, 5, 8], need)
    assert rc == 0 and total == need and list(offs) == list(want[1]) and list(status[:2]) == [0, 0] and list(ids[:need]) == list(want[0])
    # n = 0
    rc, ids, offs, status, total, bad_text = raw_encode(tok, b"", [0], 0)
    assert rc == 0 and total == 0 and list(offs) == [0] and bad_text == 0xFFFFFFFF
    # offsets need not start at 0
    rc, ids, offs, status, total, bad_text = raw_encode(tok, b"zzzab cd", [3, 5, 8], 16, special=0)
    want = s["ref"].encode(["ab", " cd"], add_special_tokens=False, max_length=0)
    assert rc == 0 and list(ids[:total]) == list(want[0]) and list(offs) == list(want[1])


def test_a_text_tokenises_alike_wherever_it_stands():
    s = state()
    tok, texts = s["tok"], s["texts"]
    want = rows(*s["want"][True][:2])
    order = np.random.default_rng(3).permutation(len(texts))
    got = tok.encode([texts[i] for i in order], max_length=0)
    assert rows(got[0], got[1]) == [want[i] for i in order]
    tok.encode(["ab [SEP]", "x" * 5000, ""], max_length=4)           # whatever the handle did before ...
    for i in (0, len(texts) // 2, len(texts) - 1):
        alone = tok.encode([texts[i]], max_length=0)
        assert rows(alone[0], alone[1]) == [want[i]]
    same_csr(tok.encode(texts, max_length=0), s["want"][True])


def test_device_output_equals_host_output():
    import torch
    s = state()
    tok, texts = s["tok"], s["texts"]
    want = s["want"][True]
    cap = len(want[0]) + 5
    ids = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    offs = torch.full((len(texts) + 1,), -1, dtype=torch.int32, device="cuda")
    status, total = tok.encode_device(texts, ids.data_ptr(), cap, offs.data_ptr(), max_length=0)
    assert total == len(want[0]) and not status.any()
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[:total], want[0])
    assert (ids.cpu().numpy()[total:] == -1).all()
    assert np.array_equal(offs.cpu().numpy().view(np.uint32), want[1])
    with pytest.raises(s["fa"].InvalidConfig):
        tok.encode_device(texts, ids.data_ptr(), total - 1, offs.data_ptr(), max_length=0)
    # pairs
    a_texts, b_texts = texts[:8], texts[8:16]
    w_ids, w_types, w_offs, w_status = s["ref"].encode_pairs(a_texts, b_texts, max_length=40)
    types = torch.full((cap,), -1, dtype=torch.int32, device="cuda")
    status, total = tok.encode_pairs_device(a_texts, b_texts, ids.data_ptr(), types.data_ptr(), cap, offs.data_ptr(), max_length=40)
    assert total == len(w_ids) and np.array_equal(status, w_status)
    assert np.array_equal(ids.cpu().numpy().view(np.uint32)[:total], w_ids)
    assert np.array_equal(types.cpu().numpy().view(np.uint32)[:total], w_types)
    assert np.array_equal(offs.cpu().numpy().view(np.uint32)[:9], w_offs)


def test_potion_embeds_raw_text_to_the_same_bits():
    import torch
    s = state()
    fa, tok = s["fa"], s["tok"]
    table = np.random.default_rng(9).standard_normal((len(s["vocab"]), 64)).astype(np.float32)
    m2v = fa.Model2VecEmbedder(table)
    texts = s["texts"]
    ids, offsets, _ = s["want"][False]   # encode_fast(text, false): no special tokens, no truncation
    want = m2v.embed_flat(np.ascontiguousarray(ids if len(ids) else np.zeros(1, np.uint32)), offsets)
    got = m2v.embed_texts(tok, texts)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert np.abs(got).sum() > 0
    out = torch.zeros((len(texts), 64), dtype=torch.float32, device="cuda")
    m2v.embed_texts_device(tok, texts, out.data_ptr())
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # a flagged text is refused with its index and the encoder is not run
    out = np.full((3, 64), 7.0, dtype=np.float32)
    with pytest.raises(fa.InvalidConfig) as err:
        m2v.embed_texts(tok, ["fine", "ab", "x [SEP] y"], out=out)
    assert err.value.bad_text == 2 and (out == 7.0).all()
    assert m2v.embed_texts(tok, []).shape == (0, 64)
    m2v.close()


def _encoder_weights(s, seed):
    """The tiny seeded BERT of the encoder tests (oracle.bert_oracle.random_weights), with the tokenizer's vocabulary size."""
    from oracle import bert_oracle
    return bert_oracle.random_weights(seed, len(s["vocab"]), 128, 2, 512)   # (hidden is a multiple of 128)


def test_minilm_embeds_raw_text_to_the_same_bits():
    import torch
    s = state()
    fa, tok, ref = s["fa"], s["tok"], s["ref"]
    m = fa.NativeEmbedder(_encoder_weights(s, 17))
    short = [t for t in s["texts"] if len(t) < 40]
    batches = {   # (texts, max_length): one per forward the embedder chooses between
        "one query (at most 32 tokens in all)": (["what is ab cd"], 0),
        "short texts (every text at most 32 tokens, more than 32 in all)": (short, 0),
        "short after truncation": (s["texts"], 32),
        "long and short texts": (s["texts"], 200),
        "empty texts": (["", ""], 0),
    }
    for what, (texts, max_length) in batches.items():
        ids, offsets, status = ref.encode(texts, add_special_tokens=True, max_length=max_length)
        assert not status.any()
        want = m.embed_flat(np.ascontiguousarray(ids.astype(np.int32)), offsets)
        for again in range(2):   # (the host-ids call replays a captured graph from its second sighting of a shape)
            got = m.embed_texts(tok, texts, max_length=max_length)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (what, again)
            assert np.array_equal(m.embed_flat(np.ascontiguousarray(ids.astype(np.int32)), offsets).view(np.uint32), want.view(np.uint32))
        assert np.isfinite(got).all() and np.abs(got).sum() > 0, what
        out = torch.zeros((len(texts), 128), dtype=torch.float32, device="cuda")
        m.embed_texts_device(tok, texts, out.data_ptr(), max_length=max_length)
        assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32)), what
    # a flagged text is refused with its index and the encoder is not run
    out = np.full((3, 128), 7.0, dtype=np.float32)
    with pytest.raises(fa.InvalidConfig) as err:
        m.embed_texts(tok, ["fine", "x [SEP] y", "ab"], out=out)
    assert err.value.bad_text == 1 and (out == 7.0).all()
    with pytest.raises(fa.InvalidConfig):   # longer than the model's positions and not truncated: as fsgpu_bert_embed
        m.embed_texts(tok, [s["texts"][s["names"].index("longer-than-the-window")]], max_length=0)
    assert m.embed_texts(tok, []).shape == (0, 128)
    # a tokenizer whose vocabulary the model cannot hold is refused
    from oracle import bert_oracle
    small = fa.NativeEmbedder(bert_oracle.random_weights(17, 100, 128, 2, 512))
    with pytest.raises(fa.InvalidConfig, match="vocabulary"):
        small.embed_texts(tok, ["ab"])
    small.close()
    m.close()


def test_reranker_scores_raw_text_to_the_same_logits():
    import reranker_ref as RR
    s = state()
    fa, tok, ref = s["fa"], s["tok"], s["ref"]
    w = _encoder_weights(s, 19)
    w.update(RR.head_weights(20, 128))
    rr = fa.NativeReranker(w)
    query = "What is ab, cd?"
    short = [t for t in s["texts"] if len(t) < 40]
    cases = {"short documents, no truncation": (query, short, 0), "all documents, truncated": (query, s["texts"], 64),
             "a budget of five pieces": (query, s["texts"], 8), "up to the model's positions": (query, s["texts"], rr.max_length),
             "an empty query": ("", short, 16)}
    for what, (q, docs, max_length) in cases.items():
        ids, types, offsets, status = ref.encode_pairs([q] * len(docs), docs, max_length=max_length)
        assert not status.any()
        want = rr.score_flat(np.ascontiguousarray(ids.astype(np.int32)), np.ascontiguousarray(types.astype(np.int32)), offsets)
        got = rr.score_texts(tok, q, docs, max_length=max_length)
        assert np.array_equal(got[0].view(np.uint32), want[0].view(np.uint32)), what
        assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), what
        assert np.isfinite(got[0]).all() and len(set(got[0].tolist())) > 1, what
    # a flagged document, and a flagged query, are refused with the pair's index
    with pytest.raises(fa.InvalidConfig) as err:
        rr.score_texts(tok, query, ["fine", "ab", "x [MASK] y"], max_length=32)
    assert err.value.bad_text == 2
    with pytest.raises(fa.InvalidConfig) as err:
        rr.score_texts(tok, "is [SEP] here", ["fine", "ab"], max_length=32)
    assert err.value.bad_text == 0
    with pytest.raises(fa.InvalidConfig):
        rr.score_texts(tok, query, ["ab"], max_length=2)
    assert rr.score_texts(tok, query, [])[0].shape == (0,)
    rr.close()

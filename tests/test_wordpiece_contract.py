"""The device WordPiece tokenizer without a GPU: tests/wordpiece_ref.py (the yardstick of test_gpu_wordpiece.py) is held to the
`tokenizers` library itself, id for id, on literals, on 20,000 seeded random strings and on the pair-truncation grid; the
tokenizer.json reader refuses what the device does not serve; and the library judges a configuration before it looks for a
device."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import wordpiece_ref as R  # noqa: E402

_STATE = {}


def state():
    """Built once per session: the code-point table (from `tokenizers`' own normalizer and pre-tokenizer), the synthetic
    vocabulary, the library's tokenizer over it and the restatement."""
    if not _STATE:
        from tokenizers import Tokenizer
        from frankensearch_amd.build import build
        build()
        from frankensearch_amd.embed import WordPieceTokenizer, bert_codepoint_table
        cp_info, expansions = bert_codepoint_table()
        vocab = R.synthetic_vocab()
        text = R.tokenizer_json(vocab)
        kw = WordPieceTokenizer.parse_tokenizer_json(text)
        kw.pop("normalizer")
        _STATE.update(cp_info=cp_info, expansions=expansions, vocab=vocab, json=text, kw=kw, hf=Tokenizer.from_str(text),
                      ref=R.WordPieceRef(cp_info=cp_info, expansions=expansions, **kw))
    return _STATE


def rows(ids, offsets):
    return [list(map(int, ids[offsets[i]:offsets[i + 1]])) for i in range(len(offsets) - 1)]


LITERALS = [
    "", " ", "a", "Hello, World!", "hello world", "héllo wörld ÀÉÎ", "İstanbul ß Σίσυφος ǅ ﬁ ẞ", "中文abc日本 語", "ab中cd",
    "한글 각 가나", "a​b a\u0000b a�b a­b", "tab\tnew\nline\r\nnbsp thin ideo　x", "...!!! ?? --", "don't stop-me [now]",
    "x" * 99, "x" * 100, "x" * 101, "é" * 100 + " " + "é" * 101, "ab" + "q" * 120 + " cd", "abzzzzzzzz\U0001f600", "a\U0001f600b \U0001f468‍\U0001f469",
    "emoji\U0001f600end", "[ CLS ] [SEP [", "ＡＢＣ ｆｕｌｌ", "ǆ Ǆ ǅ ﬀ ﬃ", "Ⅻ ⅻ ① ½",
]


def test_the_restatement_equals_tokenizers_on_the_literals():
    s = state()
    hf, ref = s["hf"], s["ref"]
    for special in (True, False):
        ids, offsets, status = ref.encode(LITERALS, add_special_tokens=special, max_length=0)
        assert not status.any()
        want = [e.ids for e in hf.encode_batch(LITERALS, add_special_tokens=special)]
        assert rows(ids, offsets) == want
    # a word that finds two pieces and then fails is ONE [UNK]; dropped characters join their neighbours; Hangul opens into jamo
    unk = s["kw"]["unk_id"]
    tid = {t: i for i, t in enumerate(s["vocab"])}
    assert ref.pieces("ab\U0001f9ff") == [unk] and hf.encode("ab\U0001f9ff", add_special_tokens=False).ids == [unk]
    assert ref.pieces("a​b") == ref.pieces("ab")
    assert ref.pieces("각")[0] == tid["ᄀ"]
    assert ref.pieces("x中y") == [tid["x"], tid["中"], tid["y"]]


def test_added_token_content_and_host_code_points_are_flagged():
    s = state()
    ref = s["ref"]
    ids, offsets, status = ref.encode(["good one", "ab [SEP] cd", "fine", "กำ ำ", "x[MASK]", "[sep] is no token"], max_length=0)
    host = [bool(int(s["cp_info"][ord(c)]) & R.WP_HOST) for c in "ำ́"]
    assert list(status) == [0, 1, 0, 1 if host[0] else 0, 1, 0]
    assert offsets[2] == offsets[1] and offsets[5] == offsets[4]          # a flagged text gets zero ids
    # HOST is what the issue says: every surviving code point with a non-zero combining class
    import unicodedata
    from tokenizers.normalizers import BertNormalizer
    keep = BertNormalizer(lowercase=True)
    for c in (0x0E33, 0x1D165, 0x302E, 0x0F39, 0x0301, 0x0E48):
        survives = [x for x in keep.normalize_str(chr(c)) if unicodedata.combining(x)]
        assert bool(int(s["cp_info"][c]) & R.WP_HOST) == bool(survives), hex(c)


def test_the_restatement_equals_tokenizers_on_twenty_thousand_random_strings():
    s = state()
    texts = R.random_strings(s["cp_info"], 20000)
    ids, offsets, status = s["ref"].encode(texts, max_length=0)
    assert int(status.sum()) == 0, "the pool holds no HOST code point and no added token"
    want = s["hf"].encode_batch(texts)
    got = rows(ids, offsets)
    mismatches = [i for i, e in enumerate(want) if e.ids != got[i]]
    assert mismatches == [], (len(mismatches), texts[mismatches[0]])
    assert sum(len(r) for r in got) > 20000 * 5


def test_pair_truncation_equals_tokenizers_on_the_grid():
    s = state()
    from tokenizers import Tokenizer
    hf = Tokenizer.from_str(s["json"])
    ref = s["ref"]
    sizes = range(0, 14)
    a_texts = [" ".join("a" * 1 for _ in range(a)) for a in sizes for _ in sizes]
    b_texts = [" ".join("b" * 1 for _ in range(b)) for _ in sizes for b in sizes]
    for max_length in (3, 4, 5, 8, 9, 16, 17):
        hf.enable_truncation(max_length)   # (longest_first, right, stride 0: the defaults)
        want = hf.encode_batch(list(zip(a_texts, b_texts)))
        ids, types, offsets, status = ref.encode_pairs(a_texts, b_texts, max_length=max_length)
        assert not status.any()
        assert rows(ids, offsets) == [e.ids for e in want], max_length
        assert rows(types, offsets) == [e.type_ids for e in want], max_length
    hf.no_truncation()
    want = hf.encode_batch(list(zip(a_texts, b_texts)))
    ids, types, offsets, _ = ref.encode_pairs(a_texts, b_texts, max_length=0)
    assert rows(ids, offsets) == [e.ids for e in want] and rows(types, offsets) == [e.type_ids for e in want]


def test_single_truncation_equals_tokenizers():
    s = state()
    from tokenizers import Tokenizer
    hf = Tokenizer.from_str(s["json"])
    texts = [" ".join("a" for _ in range(k)) for k in range(0, 12)]
    for max_length in (2, 3, 7, 8, 9):
        hf.enable_truncation(max_length)
        for special in (True, False):
            ids, offsets, _ = s["ref"].encode(texts, add_special_tokens=special, max_length=max_length)
            assert rows(ids, offsets) == [e.ids for e in hf.encode_batch(texts, add_special_tokens=special)], (max_length, special)


def test_from_tokenizer_json_refuses_other_pipelines():
    s = state()
    from frankensearch_amd.embed import WordPieceTokenizer
    table = (s["cp_info"], s["expansions"])
    import json
    good = json.loads(s["json"])

    def refused(change, match):
        doc = json.loads(s["json"])
        change(doc)
        with pytest.raises(ValueError, match=match):
            WordPieceTokenizer.from_tokenizer_json(json.dumps(doc), table=table)

    with pytest.raises(ValueError, match="BPE"):
        WordPieceTokenizer.from_tokenizer_json(R.tokenizer_json(s["vocab"], model_type="BPE"), table=table)
    with pytest.raises(ValueError, match="strategy"):
        WordPieceTokenizer.from_tokenizer_json(R.tokenizer_json(s["vocab"], max_length=16, strategy="OnlyFirst"), table=table)
    refused(lambda d: d["model"].update(type="WordLevel"), "WordLevel")
    refused(lambda d: d["model"].update(type="Unigram"), "Unigram")
    refused(lambda d: d["normalizer"].update(type="NFKC"), "normalizer")
    refused(lambda d: d["pre_tokenizer"].update(type="Whitespace"), "pre-tokenizer")
    refused(lambda d: d.update(truncation={"direction": "Left", "max_length": 8, "strategy": "LongestFirst", "stride": 0}), "direction")
    refused(lambda d: d.update(truncation={"direction": "Right", "max_length": 8, "strategy": "LongestFirst", "stride": 2}), "stride")
    refused(lambda d: d["added_tokens"][0].update(normalized=True), "normalised")
    kw = WordPieceTokenizer.parse_tokenizer_json(R.tokenizer_json(s["vocab"], max_length=16))
    assert kw["max_length"] == 16 and kw["added"] == R.ADDED and kw["prefix"] == "##" and kw["max_input_chars_per_word"] == 100
    assert kw["unk_id"] == 1 and kw["cls_id"] == 2 and kw["sep_id"] == 3 and len(kw["vocab"]) == len(good["model"]["vocab"])


def test_create_judges_the_config_before_it_looks_for_a_device():
    import torch
    import frankensearch_amd as fa
    from frankensearch_amd.embed import WP_HOST, WP_LEN_SHIFT, WordPieceTokenizer
    s = state()
    base = dict(cp_info=s["cp_info"], expansions=s["expansions"], **s["kw"])

    def create(**change):
        kw = dict(base)
        kw.update(change)
        return WordPieceTokenizer(**kw)

    def table_with(cp, value):
        t = s["cp_info"].copy()
        t[cp] = value
        return t

    vocab = s["kw"]["vocab"]
    bad = {
        "an empty vocabulary": dict(vocab=[], unk_id=0, cls_id=0, sep_id=0),
        "unk_id out of range": dict(unk_id=len(vocab)),
        "cls_id out of range": dict(cls_id=len(vocab) + 7),
        "sep_id out of range": dict(sep_id=2 ** 32 - 1),
        "two equal entries": dict(vocab=vocab[:-1] + [vocab[17]]),
        "expansion index out of range": dict(cp_info=table_with(0xAC01, len(s["expansions"]) - 1 | (3 << WP_LEN_SHIFT))),
        "output length above 3": dict(cp_info=table_with(0x41, 0x61 | (4 << WP_LEN_SHIFT))),
        "high bits": dict(cp_info=table_with(0x41, 0x61 | (1 << WP_LEN_SHIFT) | (1 << 27))),
        "a reserved word": dict(reserved=[0, 0, 5]),
        "max chars 0": dict(max_input_chars_per_word=0),
        "max chars above 1,024": dict(max_input_chars_per_word=1025),
        "a long prefix": dict(prefix="#" * 17),
        "an empty added token": dict(added=["[CLS]", ""]),
        "too many added tokens": dict(added=["[T%d]" % i for i in range(33)]),
    }
    for why, change in bad.items():
        with pytest.raises(fa.InvalidConfig):
            create(**change)
    # offsets that decrease: through the C ABI directly (the Python constructor cannot make them)
    import ctypes as C
    from frankensearch_amd import _lib
    from frankensearch_amd.embed import _WordPieceConfig, _blob
    from frankensearch_amd.errors import check
    vb, vo = _blob(vocab)
    vo = vo.copy()
    vo[5], vo[6] = vo[6], vo[5]
    ab, ao = _blob(R.ADDED)
    prefix = np.frombuffer(b"##", dtype=np.uint8).copy()
    cfg = _WordPieceConfig(vb.ctypes.data, vo.ctypes.data, len(vocab), 1, 2, 3, prefix.ctypes.data, 2, 100, s["cp_info"].ctypes.data,
                           s["expansions"].ctypes.data, s["expansions"].size, ab.ctypes.data, ao.ctypes.data, len(R.ADDED))
    h = C.c_void_p()
    with pytest.raises(fa.InvalidConfig, match="non-decreasing"):
        check(_lib.lib().fsgpu_wordpiece_create(0, C.byref(cfg), C.byref(h)))
    # ... and a good config then asks for the GPU
    if torch.cuda.is_available():
        tok = create()
        assert tok.vocab_size() == len(vocab)
        tok.close()
    else:
        with pytest.raises(fa.NoDevice):
            create()
    # an entry longer than its code point's UTF-8 form is accepted and treated as HOST (include/fsgpu.h); the restatement agrees
    t = table_with(0x41, 0 | (2 << WP_LEN_SHIFT))
    ref = R.WordPieceRef(cp_info=t, expansions=s["expansions"], **s["kw"])
    assert ref.pieces("bAb") is None and ref.pieces("bab") is not None and not int(t[0x41]) & WP_HOST

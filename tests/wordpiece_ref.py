"""A plain-Python restatement of the device WordPiece tokenizer (fsgpu_wordpiece_*), working from the blobs and
tables the C ABI receives: the vocabulary blob and its offsets, cp_info and the expansions, the added tokens' contents.  It
never calls `tokenizers`; tests compare it with that library on one side and with the device on the other.

Also the shared fixtures of the two test files: the synthetic vocabularies, the pool the random strings are drawn from and a
tokenizer.json writer."""
import json

import numpy as np

# cp_info's bit layout, restated from include/fsgpu.h (not imported from the package under test)
WP_VALUE_MASK = 0x1FFFFF
WP_LEN_SHIFT = 21
WP_SPACE = 1 << 24
WP_ISOLATE = 1 << 25
WP_HOST = 1 << 26


def _blob(items):
    """Byte strings -> (uint8 blob, uint32 offsets [len + 1]): the C ABI's shape for the vocabulary and the added tokens."""
    raw = [x if isinstance(x, (bytes, bytearray)) else str(x).encode("utf-8") for x in items]
    offsets = np.zeros(len(raw) + 1, dtype=np.uint32)
    for i, b in enumerate(raw):
        offsets[i + 1] = offsets[i] + len(b)
    return np.frombuffer(b"".join(raw) or b"\0", dtype=np.uint8).copy(), offsets


def _utf8_len(c):
    return 1 if c < 0x80 else 2 if c < 0x800 else 3 if c < 0x10000 else 4


class WordPieceRef:
    def __init__(self, vocab, unk_id, cls_id, sep_id, cp_info, expansions, added=(), prefix="##", max_input_chars_per_word=100,
                 max_length=0, **_):
        self.vocab_bytes, self.vocab_offsets = _blob(vocab)
        blob = self.vocab_bytes.tobytes()
        off = self.vocab_offsets
        self.index = {blob[off[i]:off[i + 1]]: i for i in range(len(off) - 1)}   # bytes -> id (entries are distinct)
        self.added_bytes, self.added_offsets = _blob(added)
        ab, ao = self.added_bytes.tobytes(), self.added_offsets
        self.added = [ab[ao[i]:ao[i + 1]] for i in range(len(ao) - 1)]
        self.prefix = prefix.encode("utf-8") if isinstance(prefix, str) else bytes(prefix)
        self.cp_info = np.asarray(cp_info, dtype=np.uint32)
        self.expansions = [int(x) for x in np.asarray(expansions, dtype=np.uint32)]
        self.unk_id, self.cls_id, self.sep_id = unk_id, cls_id, sep_id
        self.max_chars = max_input_chars_per_word
        self.max_length = max_length
        self._memo = {}

    def words(self, raw: bytes):
        """The text's words as lists of normalised code points, or None when the text is flagged."""
        if any(a in raw for a in self.added):
            return None
        words, cur = [], []
        info_of, memo = self.cp_info, self._memo
        for ch in raw.decode("utf-8"):
            c = ord(ch)
            info = memo.get(c)
            if info is None:
                info = memo[c] = int(info_of[c])
            n = (info >> WP_LEN_SHIFT) & 7
            if info & WP_HOST or n > min(3, _utf8_len(c)):
                return None
            if n == 0:
                continue
            v = info & WP_VALUE_MASK
            if n > 1:
                cur.extend(self.expansions[v:v + n])
            elif info & (WP_SPACE | WP_ISOLATE):
                if cur:
                    words.append(cur)
                    cur = []
                if not info & WP_SPACE:
                    words.append([v])
            else:
                cur.append(v)
        if cur:
            words.append(cur)
        return words

    def word_pieces(self, word):
        if len(word) > self.max_chars:
            return [self.unk_id]
        enc = [chr(v).encode("utf-8") for v in word]
        out, start = [], 0
        while start < len(word):
            for end in range(len(word), start, -1):
                found = self.index.get((self.prefix if start else b"") + b"".join(enc[start:end]))
                if found is not None:
                    break
            else:
                return [self.unk_id]
            out.append(found)
            start = end
        return out

    def pieces(self, text):
        raw = text if isinstance(text, (bytes, bytearray)) else text.encode("utf-8")
        words = self.words(bytes(raw))
        if words is None:
            return None
        return [p for w in words for p in self.word_pieces(w)]

    @staticmethod
    def _csr(rows):
        offsets = np.zeros(len(rows) + 1, dtype=np.uint32)
        offsets[1:] = np.cumsum([len(r) for r in rows])
        flat = np.asarray([x for r in rows for x in r], dtype=np.uint32)
        return flat, offsets

    def encode(self, texts, add_special_tokens=True, max_length=None):
        max_length = self.max_length if max_length is None else max_length
        rows, status = [], []
        for t in texts:
            p = self.pieces(t)
            status.append(1 if p is None else 0)
            if p is None:
                rows.append([])
                continue
            sp = 2 if add_special_tokens else 0
            if max_length:
                p = p[:max_length - sp]
            rows.append([self.cls_id] + p + [self.sep_id] if sp else p)
        ids, offsets = self._csr(rows)
        return ids, offsets, np.asarray(status, dtype=np.uint8)

    @staticmethod
    def pair_keep(la, lb, max_length):
        """longest_first on the budget max_length - 3, in closed form (include/fsgpu.h)."""
        if not max_length:
            return la, lb
        budget = max_length - 3
        if la + lb <= budget:
            return la, lb
        swap = la > lb
        n1, n2 = (lb, la) if swap else (la, lb)
        n2 = n1 if n1 > budget else max(n1, budget - n1)
        if n1 + n2 > budget:
            n1 = budget // 2
            n2 = n1 + budget % 2
        return (n2, n1) if swap else (n1, n2)

    def encode_pairs(self, a_texts, b_texts, max_length=None):
        max_length = self.max_length if max_length is None else max_length
        rows, types, status = [], [], []
        for ta, tb in zip(a_texts, b_texts):
            pa, pb = self.pieces(ta), self.pieces(tb)
            if pa is None or pb is None:
                status.append(1)
                rows.append([])
                types.append([])
                continue
            status.append(0)
            ka, kb = self.pair_keep(len(pa), len(pb), max_length)
            rows.append([self.cls_id] + pa[:ka] + [self.sep_id] + pb[:kb] + [self.sep_id])
            types.append([0] * (ka + 2) + [1] * (kb + 1))
        ids, offsets = self._csr(rows)
        return ids, self._csr(types)[0], offsets, np.asarray(status, dtype=np.uint8)


# ---- fixtures both test files share ----

ADDED = ["[PAD]", "[UNK]", "[CLS]", "[SEP]", "[MASK]"]
LETTERS = "abcdefghijklmnopqrstuvwxyz"
PUNCT = list("!\"#$%&'()*+,-./:;<=>?@[\\]^_`{|}~") + ["¡", "¿", "—", "。", "،"]
CJK = list("中文字日本語漢")
JAMO = [chr(c) for c in list(range(0x1100, 0x1113)) + list(range(0x1161, 0x1176)) + list(range(0x11a8, 0x11c3))]
OTHER = list("ßσςıǆﬁæøджαβ") + ["\U0001f600", "\U0001f44d", "\U00010400", "\U00010428"]


def synthetic_vocab(seed=7, size=3000):
    """~3,000 entries: the added tokens, single letters and digits with their ## forms, punctuation, CJK, jamo and a few
    other characters, then random lowercase pieces (half of them ## pieces) of 2..6 letters."""
    rng = np.random.default_rng(seed)
    vocab = list(ADDED)
    singles = list(LETTERS) + list("0123456789") + JAMO + OTHER
    vocab += singles + ["##" + s for s in singles] + PUNCT + CJK
    seen = set(vocab)
    while len(vocab) < size:
        w = "".join(rng.choice(list(LETTERS), size=int(rng.integers(2, 7))))
        if rng.random() < 0.5:
            w = "##" + w
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    return vocab


def random_vocab(seed=11, size=30522):
    """30,522 entries of random pieces: the hash table at the size of the real models' vocabularies."""
    rng = np.random.default_rng(seed)
    vocab = list(ADDED) + list(LETTERS) + ["##" + c for c in LETTERS]
    seen = set(vocab)
    alphabet = list(LETTERS) + list("0123456789") + JAMO[:8] + list("ßдα")
    while len(vocab) < size:
        w = "".join(rng.choice(alphabet, size=int(rng.integers(1, 8))))
        if rng.random() < 0.5:
            w = "##" + w
        if w not in seen:
            seen.add(w)
            vocab.append(w)
    return vocab


def tokenizer_json(vocab, max_length=None, model_type="WordPiece", strategy="LongestFirst", lowercase=True):
    """The text of a tokenizer.json with the BERT pipeline around `vocab` (ids in list order)."""
    tid = {t: i for i, t in enumerate(vocab)}
    special = lambda t, ty: {"SpecialToken": {"id": t, "type_id": ty}}
    seq = lambda s, ty: {"Sequence": {"id": s, "type_id": ty}}
    doc = {
        "version": "1.0",
        "truncation": None if max_length is None else {"direction": "Right", "max_length": max_length, "strategy": strategy, "stride": 0},
        "padding": None,
        "added_tokens": [{"id": tid[t], "content": t, "single_word": False, "lstrip": False, "rstrip": False, "normalized": False,
                          "special": True} for t in ADDED],
        "normalizer": {"type": "BertNormalizer", "clean_text": True, "handle_chinese_chars": True, "strip_accents": None,
                       "lowercase": lowercase},
        "pre_tokenizer": {"type": "BertPreTokenizer"},
        "post_processor": {"type": "TemplateProcessing",
                           "single": [special("[CLS]", 0), seq("A", 0), special("[SEP]", 0)],
                           "pair": [special("[CLS]", 0), seq("A", 0), special("[SEP]", 0), seq("B", 1), special("[SEP]", 1)],
                           "special_tokens": {t: {"id": t, "ids": [tid[t]], "tokens": [t]} for t in ("[CLS]", "[SEP]")}},
        "decoder": None,
        "model": {"type": model_type, "unk_token": "[UNK]", "continuing_subword_prefix": "##", "max_input_chars_per_word": 100,
                  "vocab": tid},
    }
    if model_type == "BPE":
        doc["model"] = {"type": "BPE", "vocab": tid, "merges": []}
    return json.dumps(doc)


def string_pool(cp_info):
    """What the random strings are made of: ASCII, accents, case and width oddities, CJK, Hangul, zero-width and control
    characters, U+FFFD, emoji — with every HOST-class code point taken out ('[' stays: no string gets an added token's content
    because ']' never follows the names, see random_strings)."""
    chars = (list(LETTERS) * 4 + list(LETTERS.upper()) + list("0123456789") + [" "] * 12 + ["\t", "\n", "\r", " ", "　"] +
             list("éèüñåÅÇşİßΣσςǅﬁйЙẞΐ") +
             PUNCT + CJK + ["豈", "\U0002f800"] + list("각한글가") + JAMO[:6] +
             ["​", "‍", "﻿", "\u0000", "\u0007", "\u007f", "�", "­", "\U0001f600", "\U0001f468", "́",
              "̈", "ำ", "ொ"])
    return [c for c in chars if not int(cp_info[ord(c)]) & WP_HOST]


def random_strings(cp_info, count, seed=1234):
    rng = np.random.default_rng(seed)
    pool = np.asarray(string_pool(cp_info), dtype=object)
    out = []
    for i in range(count):
        if i % 50 == 0:   # a word of 95..105 characters among ordinary ones
            word = "".join(rng.choice(pool[:26], size=int(rng.integers(95, 106))))
            s = "".join(rng.choice(pool, size=int(rng.integers(0, 12)))) + " " + word + " " + "".join(rng.choice(pool, size=int(rng.integers(0, 12))))
        else:
            s = "".join(rng.choice(pool, size=int(rng.integers(0, 60))))
        for a in ADDED:   # (a random draw that spells an added token: take it apart)
            s = s.replace(a, a[:-1] + " ")
        out.append(s)
    return out

"""CPU checks of the cross-encoder reranker's contract: the f32 restatement (tests/reranker_ref.py) against the transformers golden,
the safetensors rules of fsgpu_reranker_create_safetensors (checked before a device is looked for), and fsgpu_rerank_apply — the host
step after the model call — against the reference's inline tests (crates/frankensearch-rerank/src/pipeline.rs) and a restatement."""
import json
import math
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import reranker_ref as R  # noqa: E402


def _golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "reranker_golden.npz"))


def golden_case(name):
    from oracle import bert_oracle
    g = _golden()
    vocab, hidden, layers, inter, ws, hs, _ = [int(v) for v in g[f"{name}_config"]]
    w = bert_oracle.random_weights(ws, vocab, hidden, layers, inter)
    w.update(R.head_weights(hs, hidden))
    lens = g[f"{name}_lengths"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    pairs = [(g[f"{name}_ids"][offs[i]:offs[i + 1]].tolist(), g[f"{name}_types"][offs[i]:offs[i + 1]].astype(int).tolist())
             for i in range(len(lens))]
    return w, pairs, g[f"{name}_logits"]


@pytest.mark.parametrize("name", ["tiny", "minilm"])
def test_restatement_matches_transformers_golden(name):
    w, pairs, want = golden_case(name)
    assert max(len(p[0]) for p in pairs) == 512 and min(len(p[0]) for p in pairs) == 3
    assert any(1 in p[1] for p in pairs) and any(p[1].count(1) == 2 for p in pairs)   # both types; a 1-token doc segment
    got = R.logits(w, pairs)
    assert np.max(np.abs(got - want)) <= 1e-4 * max(1.0, float(np.max(np.abs(want)))), (got, want)


# ---- fsgpu_reranker_create_safetensors: blob rules, checked without a device -------------------------------------------------
def _blob(tensors):
    header, data, off = {}, b"", 0
    for name, arr in tensors.items():
        a = np.ascontiguousarray(arr, dtype=np.float32)
        header[name] = {"dtype": "F32", "shape": list(a.shape), "data_offsets": [off, off + a.nbytes]}
        data += a.tobytes()
        off += a.nbytes
    h = json.dumps(header).encode()
    h += b" " * ((8 - len(h) % 8) % 8)
    return struct.pack("<Q", len(h)) + h + data


def _tiny_weights(bare=True):
    from oracle import bert_oracle
    w = bert_oracle.random_weights(3, 64, 128, 1, 512, max_pos=64)
    if not bare:
        w = {("bert." + k): v for k, v in w.items()}
    w.update(R.head_weights(4, 128))
    return w


def _create(blob):
    import ctypes as C
    import frankensearch_amd as fa
    from frankensearch_amd.errors import check
    buf = np.frombuffer(blob, dtype=np.uint8).copy()
    h = C.c_void_p()
    st = fa._lib.lib().fsgpu_reranker_create_safetensors(-1, buf.ctypes.data, buf.size, 0.0, C.byref(h))
    if st == 0 and h.value:
        fa._lib.lib().fsgpu_reranker_destroy(h)
    check(st)


@pytest.mark.parametrize("drop", ["bert.pooler.dense.weight", "bert.pooler.dense.bias", "classifier.weight", "classifier.bias"])
def test_blob_without_head_tensor_is_model_load_failed(drop):
    import frankensearch_amd as fa
    w = _tiny_weights()
    del w[drop]
    with pytest.raises(fa.ModelLoadFailed, match="missing tensor " + drop.replace(".", r"\.")):
        _create(_blob(w))


def test_blob_with_two_row_classifier_is_model_load_failed():
    import frankensearch_amd as fa
    w = _tiny_weights()
    w["classifier.weight"] = np.ones((2, 128), np.float32)
    w["classifier.bias"] = np.zeros(2, np.float32)
    with pytest.raises(fa.ModelLoadFailed, match="expected 1 logits, got 2"):
        _create(_blob(w))


@pytest.mark.parametrize("bare", [True, False])
def test_blob_with_bare_or_prefixed_keys_passes_validation(bare):
    import frankensearch_amd as fa
    # a valid blob gets past the parse: the device lookup comes next (device -1 is never a device)
    with pytest.raises((fa.InvalidConfig, fa.NoDevice)):
        _create(_blob(_tiny_weights(bare)))


# ---- fsgpu_rerank_apply vs the inline tests of pipeline.rs ---------------------------------------------------------------------
def make_candidates(n):
    from frankensearch_amd.rerank import RerankCandidate
    return [RerankCandidate(f"doc-{i}", float(np.float32(i) * np.float32(-0.1) + np.float32(1.0)), None, i) for i in range(n)]


def text_for_doc(doc_id):
    return True


def text_for_doc_partial(doc_id):
    return int(doc_id.split("-")[1]) % 2 == 0


def stub_scores(n):   # StubReranker: 1 - i / len
    ln = max(n, 1)
    return [float(np.float32(1.0) - np.float32(i) / np.float32(ln)) for i in range(n)]


def false_positive_scores(n):   # FalsePositiveReranker: the deepest document gets 1.0
    return [1.0 if i + 1 == n else float(np.float32(i) * np.float32(-0.01) + np.float32(0.9)) for i in range(n)]


def step(cands, text_fn, top_k, min_c, scorer=stub_scores, combine=0, k=60.0):
    """rerank_step_with_combine with a stub model: the host half through fsgpu_rerank_apply."""
    from frankensearch_amd.rerank import rerank_apply
    if len(cands) < min_c:
        return cands, False
    window = min(len(cands), top_k)
    has = [text_fn(c.doc_id) for c in cands[:window]]
    n_text = sum(has)
    if n_text < min_c:
        return cands, False
    return rerank_apply(cands, has + [False] * (len(cands) - window), scorer(n_text), top_k, min_c, combine, k)


def test_rerank_happy_path():
    out, applied = step(make_candidates(10), text_for_doc, 100, 5)
    assert applied and all(c.rerank_score is not None for c in out)


def test_rerank_too_few_candidates():
    c = make_candidates(3)
    out, applied = step(c, text_for_doc, 100, 5)
    assert not applied and [x.score for x in out] == [x.score for x in c]
    from frankensearch_amd.rerank import rerank_apply
    out, applied = rerank_apply(c, [True] * 3, stub_scores(3), 100, 5)   # the library makes the same check
    assert not applied and all(x.rerank_score is None for x in out)


def test_rerank_missing_text():
    out, applied = step(make_candidates(10), text_for_doc_partial, 100, 5)
    assert applied
    for c in out:
        if int(c.doc_id.split("-")[1]) % 2 == 0:
            assert c.rerank_score is not None, c.doc_id


def test_rerank_missing_text_clears_stale_scores_for_non_reranked_candidates():
    c = make_candidates(6)
    for x in c:
        x.rerank_score = 999.0
    out, applied = step(c, text_for_doc_partial, 6, 3)
    assert applied
    for x in out:
        if int(x.doc_id.split("-")[1]) % 2 == 0:
            assert x.rerank_score is not None and x.rerank_score != 999.0
        else:
            assert x.rerank_score is None


def test_rerank_missing_text_below_threshold():
    out, applied = step(make_candidates(6), text_for_doc_partial, 100, 5)
    assert not applied and all(c.rerank_score is None for c in out)
    from frankensearch_amd.rerank import rerank_apply
    out, applied = rerank_apply(make_candidates(6), [text_for_doc_partial(f"doc-{i}") for i in range(6)], stub_scores(3), 100, 5)
    assert not applied and all(c.rerank_score is None for c in out)


def test_rerank_respects_top_k():
    out, applied = step(make_candidates(20), text_for_doc, 10, 5)
    assert applied
    for i, c in enumerate(out):
        assert (c.rerank_score is not None) == (i < 10), i


def test_rerank_tie_breaks_by_doc_id():
    c = make_candidates(6)
    c.reverse()   # (arrival order must not matter)
    out, applied = step(c, text_for_doc, 100, 5, scorer=lambda n: [0.5] * n)
    assert applied
    ids = [x.doc_id for x in out]
    assert ids == sorted(ids)


def test_non_reranked_candidates_keep_original_order():
    c = make_candidates(15)
    tail = [x.doc_id for x in c[10:]]
    out, applied = step(c, text_for_doc, 10, 5)
    assert applied and [x.doc_id for x in out[10:]] == tail and all(x.rerank_score is None for x in out[10:])


def test_rerank_min_candidates_zero_always_proceeds():
    out, applied = step(make_candidates(2), text_for_doc, 100, 0)
    assert applied and all(c.rerank_score is not None for c in out)


def test_rerank_top_k_zero_reranks_nothing():
    c = make_candidates(10)
    out, applied = step(c, text_for_doc, 0, 0)
    assert applied and all(x.rerank_score is None for x in out) and [x.doc_id for x in out] == [x.doc_id for x in c]


def test_rerank_overwrites_pre_existing_rerank_score():
    c = make_candidates(6)
    for x in c:
        x.rerank_score = 999.0
    out, applied = step(c, text_for_doc, 100, 5)
    assert applied and all(x.rerank_score is not None and x.rerank_score != 999.0 for x in out)


def test_rrf_combine_vetoes_deep_false_positive():
    pure, _ = step(make_candidates(5), text_for_doc, 100, 2, scorer=false_positive_scores)
    assert pure[0].doc_id == "doc-4"
    rrf, applied = step(make_candidates(5), text_for_doc, 100, 2, scorer=false_positive_scores, combine=1, k=60.0)
    assert applied and rrf[0].doc_id == "doc-0" and all(c.rerank_score is not None for c in rrf)


def test_rrf_combine_order_vector_matches_reference_permutation():
    c = make_candidates(16)
    scores, has = [], []
    for i in range(16):
        s = float(np.float32((i * 13 + 7) % 17) * np.float32(0.1))
        scores.append(float("nan") if i % 7 == 0 else s)   # None in the reference: a non-finite score is skipped -> None
        has.append(True)
    from frankensearch_amd.rerank import rerank_apply
    out, applied = rerank_apply(c, has, scores, 100, 0, 1, 60.0)
    ref, _ = R.apply_ref([{"doc_id": x.doc_id.encode(), "rerank_score": float("nan")} for x in c], has, scores, 100, 0, 1, 60.0)
    assert applied and [x.doc_id.encode() for x in out] == [r["doc_id"] for r in ref]
    for x, r in zip(out, ref):
        assert (x.rerank_score is None and math.isnan(r["rerank_score"])) or x.rerank_score == r["rerank_score"]


def test_rerank_apply_matches_restatement_on_random_cases():
    from frankensearch_amd.rerank import RerankCandidate, rerank_apply
    rng = np.random.default_rng(7)
    specials = [float("nan"), float("inf"), float("-inf"), 0.0, -0.0]
    for case in range(400):
        n = int(rng.integers(0, 24))
        ids = [f"d{int(rng.integers(0, 12))}" for _ in range(n)]   # duplicates: the tie-breaks matter
        cands = [RerankCandidate(ids[i], float(rng.standard_normal()),
                                 None if rng.random() < 0.5 else float(np.float32(rng.standard_normal())), i) for i in range(n)]
        top_k = int(rng.integers(0, 30))
        min_c = int(rng.integers(0, 6))
        window = min(n, top_k)
        has = [bool(rng.random() < 0.8) for _ in range(n)]
        n_text = sum(has[:window])
        scores = []
        for _ in range(n_text):
            r = rng.random()
            scores.append(specials[int(rng.integers(0, 5))] if r < 0.2 else
                          float(np.float32(round(rng.random() * 4) / 4)) if r < 0.5 else float(np.float32(rng.random())))
        if case % 17 == 0 and scores:
            scores = scores[:-1]   # a count mismatch is skipped
        combine = int(rng.integers(0, 2))
        k = [60.0, 0.5, -3.0, float("nan"), 1.0, 0.0][case % 6]
        out, applied = rerank_apply(cands, has, scores, top_k, min_c, combine, k)
        ref, ref_applied = R.apply_ref(
            [{"doc_id": c.doc_id.encode(), "rerank_score": float("nan") if c.rerank_score is None else c.rerank_score, "i": c.index}
             for c in cands], has, scores, top_k, min_c, combine, k)
        assert applied == ref_applied, case
        assert [c.index for c in out] == [r["i"] for r in ref], case
        for c, r in zip(out, ref):
            assert (c.rerank_score is None and math.isnan(r["rerank_score"])) or \
                np.float32(c.rerank_score).view(np.uint32) == np.float32(r["rerank_score"]).view(np.uint32), case

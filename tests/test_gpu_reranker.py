"""The GPU cross-encoder reranker (fsgpu_reranker_*, bert_rerank.hip + the embedder's fragment-order layers) against the
transformers golden and the f32 restatement (tests/reranker_ref.py).

Tolerances: logits |d| <= 2e-2 * max(1, |ref|), scores |d| <= 5e-3 (f16 matrix-core linears against f32).  Measured maxima on MI355X
(gfx950), printed by the tests: relative logit 5.96e-3 and score 1.29e-3 (MiniLM shape vs transformers); tiny shape 5.5e-4 / 1.0e-4;
heavy-tailed weights 2.8e-4 / 6.1e-5."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, ROOT)

import reranker_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

LOGIT_TOL = 2e-2
SCORE_TOL = 5e-3


def _golden_case(name):
    from oracle import bert_oracle
    g = np.load(os.path.join(ROOT, "tests", "golden", "reranker_golden.npz"))
    vocab, hidden, layers, inter, ws, hs, _ = [int(v) for v in g[f"{name}_config"]]
    w = bert_oracle.random_weights(ws, vocab, hidden, layers, inter)
    w.update(R.head_weights(hs, hidden))
    lens = g[f"{name}_lengths"]
    offs = np.concatenate([[0], np.cumsum(lens)])
    pairs = [(g[f"{name}_ids"][offs[i]:offs[i + 1]].tolist(), g[f"{name}_types"][offs[i]:offs[i + 1]].astype(int).tolist())
             for i in range(len(lens))]
    return w, pairs, g[f"{name}_logits"]


_MODELS = {}


def _model(name, heavy=False):
    import frankensearch_amd as fa
    key = (name, heavy)
    if key not in _MODELS:
        if heavy:
            from oracle import bert_oracle
            vocab, hidden, layers, inter = (500, 128, 2, 512) if name == "tiny" else (30522, 384, 6, 1536)
            w = bert_oracle.heavy_tailed_weights(31, vocab, hidden, layers, inter)
            w.update(R.head_weights(32, hidden))
        else:
            w = _golden_case(name)[0]
        _MODELS[key] = (w, fa.NativeReranker(w, device=0))
    return _MODELS[key]


def _check(got_l, got_s, ref_l, what):
    ref_l = np.asarray(ref_l, np.float32)
    dl = np.abs(got_l - ref_l) / np.maximum(1.0, np.abs(ref_l))
    ds = np.abs(got_s - R.scores_of(ref_l))
    print(f"{what}: max rel logit diff {dl.max():.3e}, max score diff {ds.max():.3e}")
    assert dl.max() <= LOGIT_TOL, (what, dl.max(), got_l, ref_l)
    assert ds.max() <= SCORE_TOL, (what, ds.max())


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32)


@pytest.mark.parametrize("name", ["tiny", "minilm"])
def test_golden_and_restatement(name):
    w, pairs, want = _golden_case(name)
    _, m = _model(name)
    lg, sc = m.score_pairs(pairs)
    _check(lg, sc, want, f"{name} vs transformers")
    _check(lg, sc, R.logits(w, pairs), f"{name} vs restatement")


@pytest.mark.parametrize("name", ["tiny", "minilm"])
@pytest.mark.parametrize("heavy", [False, True])
def test_ragged_batches_both_types(name, heavy):
    w, m = _model(name, heavy)
    vocab = w["embeddings.word_embeddings.weight"].shape[0]
    rng = np.random.default_rng(5)
    pairs = []
    for total in [3, 4, 17, 33, 64, 130, 255, 300, 511, 512]:
        q = int(rng.integers(0, min(total - 3, 30) + 1))
        pairs.append(R.make_pair(rng, vocab, q, total - q - 3))
    assert sorted(len(p[0]) for p in pairs)[0] == 3 and max(len(p[0]) for p in pairs) == 512
    lg, sc = m.score_pairs(pairs)
    ref = R.logits(w, pairs)
    _check(lg, sc, ref, f"{name} heavy={heavy} ragged")
    # ranking: the GPU order equals the restatement's wherever reference logits are more than twice the tolerance apart
    for i in range(len(pairs)):
        for j in range(len(pairs)):
            if ref[i] - ref[j] > 2 * LOGIT_TOL * max(1.0, abs(ref[i]), abs(ref[j])):
                assert lg[i] > lg[j], (i, j, ref[i], ref[j], lg[i], lg[j])


def test_token_types_matter():
    w, m = _model("minilm")
    rng = np.random.default_rng(9)
    ids, types = R.make_pair(rng, 30522, 8, 40)
    zeros = [0] * len(ids)
    lg, sc = m.score_pairs([(ids, types), (ids, zeros)])
    assert lg[0] != lg[1]
    ref = R.logits(w, [(ids, types), (ids, zeros)])
    _check(lg, sc, ref, "types vs all-zero types")


def test_bitwise_batch_invariance():
    w, m = _model("minilm")
    rng = np.random.default_rng(11)
    pairs = []
    for _ in range(100):
        total = int(rng.integers(3, 300))
        q = int(rng.integers(0, min(total - 3, 20) + 1))
        pairs.append(R.make_pair(rng, 30522, q, total - q - 3))
    full_l, full_s = m.score_pairs(pairs)
    for i in (0, 1, 37, 99):
        al, as_ = m.score_pairs([pairs[i]])
        assert _bits(al)[0] == _bits(full_l)[i] and _bits(as_)[0] == _bits(full_s)[i], i
    rl, rs = m.score_pairs(pairs[::-1])
    assert np.array_equal(_bits(rl[::-1]), _bits(full_l)) and np.array_equal(_bits(rs[::-1]), _bits(full_s))
    parts = [m.score_pairs(pairs[a:b]) for a, b in ((0, 13), (13, 64), (64, 100))]
    assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(full_l))


def test_large_call_equals_its_parts():
    w, m = _model("minilm")
    rng = np.random.default_rng(13)
    pairs = [R.make_pair(rng, 30522, 20, 512 - 23) for _ in range(100)]
    lg, sc = m.score_pairs(pairs)
    parts = [m.score_pairs(pairs[a:a + 10]) for a in range(0, 100, 10)]
    assert np.array_equal(_bits(np.concatenate([p[0] for p in parts])), _bits(lg))
    assert np.array_equal(_bits(np.concatenate([p[1] for p in parts])), _bits(sc))
    _check(lg[:3], sc[:3], R.logits(w, pairs[:3]), "100 x 512 (first three)")


def test_errors_and_empty_inputs():
    import frankensearch_amd as fa
    w, m = _model("tiny")
    assert m.max_length == 512
    ok = ([101, 7, 102, 9, 102], [0, 0, 0, 1, 1])
    with pytest.raises(fa.InvalidConfig):
        m.score_pairs([ok, ([101] * 513, [0] * 513)])
    with pytest.raises(fa.InvalidConfig):
        m.score_pairs([ok, ([101, 500, 102], [0, 0, 0])])
    with pytest.raises(fa.InvalidConfig):
        m.score_pairs([ok, ([101, 5, 102], [0, 2, 0])])
    lg, sc = m.score_pairs([])
    assert lg.shape == (0,) and sc.shape == (0,)
    lg, sc = m.score_pairs([ok, ([], []), ok])
    assert lg[1] == 0.0 and sc[1] == 0.5
    alone, _ = m.score_pairs([ok])
    assert _bits(lg)[0] == _bits(alone)[0] == _bits(lg)[2]


def test_blob_equals_struct():
    import frankensearch_amd as fa
    from test_reranker_contract import _blob
    w, m = _model("tiny")
    blob = _blob(w)
    mb = fa.NativeReranker.from_safetensors_bytes(blob, device=0)
    _, pairs, _ = _golden_case("tiny")
    a, _ = m.score_pairs(pairs)
    b, _ = mb.score_pairs(pairs)
    assert np.array_equal(_bits(a), _bits(b))
    mb.close()


def test_rerank_step_end_to_end():
    from frankensearch_amd.rerank import PURE_REORDER, RRF_COMBINE, RerankCandidate, rerank_step
    w, m = _model("tiny")
    rng = np.random.default_rng(17)
    docs = {f"doc-{i}": (R.make_pair(rng, 500, 5, int(rng.integers(1, 60))) if i % 4 != 3 else None) for i in range(12)}
    cands = [RerankCandidate(d, 1.0 - 0.05 * i, None, i) for i, d in enumerate(docs)]
    for combine in (PURE_REORDER, RRF_COMBINE):
        out, applied, err = rerank_step(m, cands, docs.get, top_k_rerank=10, min_candidates=5, combine=combine, k=60.0)
        assert err is None and applied
        window = cands[:10]
        with_text = [c for c in window if docs[c.doc_id] is not None]
        _, scores = m.score_pairs([docs[c.doc_id] for c in with_text])
        ref, ok = R.apply_ref([{"doc_id": c.doc_id.encode(), "rerank_score": float("nan"), "i": c.index} for c in cands],
                              [docs[c.doc_id] is not None for c in cands], [float(s) for s in scores], 10, 5, combine, 60.0)
        assert ok and [c.index for c in out] == [r["i"] for r in ref]
    # a scoring error (an id past the vocabulary) leaves the candidates as they were and is returned
    bad = dict(docs)
    bad["doc-0"] = ([101, 9999, 102], [0, 0, 0])
    out, applied, err = rerank_step(m, cands, bad.get, top_k_rerank=10, min_candidates=5)
    assert err is not None and not applied and [c.doc_id for c in out] == [c.doc_id for c in cands]

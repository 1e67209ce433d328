"""No GPU: fsgpu_lab_bert_int8_stage and the CLS_HEAD stage are declared, exported and bound and refuse bad shapes before a device is
looked for; the references of tests/int8_stage_ref.py agree with the f32 oracles; the exact restatements give hand-computed answers;
and the comparator is not blind — on the inputs of tests/test_gpu_int8_stages.py a mutated reference standing in for the GPU must fail
its check (for a bounded stage: reach 10 x the stage's factor), while the reference evaluated in f32 numpy stays inside its own bound."""
import os
import re

import numpy as np
import pytest

import encoder_stage_ref as E
import int8_dynamic_ref as Q
import int8_stage_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BLIND = 10.0
F = np.float32


def test_lab_entry_is_declared_exported_and_bound():
    import ctypes
    from frankensearch_amd import _lib
    from frankensearch_amd.build import build
    build()
    text = open(os.path.join(ROOT, "include", "fsgpu_lab.h")).read()
    assert re.search(r"fsgpu_status fsgpu_lab_bert_int8_stage\(int32_t device, const fsgpu_lab_bert_int8_stage_args \*args\);", text)
    assert "fsgpu_lab_bert_int8_stage" in _lib.SIGNATURES and hasattr(ctypes.CDLL(_lib.LIB_PATH), "fsgpu_lab_bert_int8_stage")
    body = re.search(r"typedef struct fsgpu_lab_bert_int8_stage_args \{(.*?)\}", text, re.S).group(1)
    names = re.findall(r"[\s*,]\*?([a-z_0-9]+)(?:\[5\])?[,;]", body)
    assert names == [n.rstrip("_") for n, _ in _lib.BertInt8StageArgs._fields_], names
    # nine u32, a float, three pointers, five inputs, three outputs
    assert ctypes.sizeof(_lib.BertInt8StageArgs) == 9 * 4 + 4 + 11 * 8
    for name, value in (("QUANT_ROWS", R.QUANT_ROWS), ("PACK_W", R.PACK_W), ("GEMM", R.GEMM), ("EMBED_LN_QUANT", R.EMBED_LN_QUANT),
                        ("ADD_LN_QUANT", R.ADD_LN_QUANT)):
        assert re.search(rf"#define FSGPU_LAB_BERT_I8_{name} {value}\n", text)
    assert re.search(rf"#define FSGPU_LAB_BERT_CLS_HEAD {R.CLS_HEAD}\n", text)


def test_bad_arguments_are_refused_before_a_device_is_looked_for():
    from frankensearch_amd.build import build
    build()
    z = lambda *shape: np.zeros(shape, F)
    bad, null = 2, 8
    # N or K not a multiple of 64, K above the cap
    for n, k in ((96, 64), (64, 96), (64, 4160), (64, 8192), (0, 64)):
        assert R.run_int8_stage(R.PACK_W, 0, [z(max(n, 1), k)], q_shape=(max(n, 1) * k,), n=n, k=k, expect=bad) == bad
        assert R.run_int8_stage(R.GEMM, 0, [z(2), z(max(n, 1), k), z(max(n, 1))], codes=np.zeros((2, k), np.int8), f32_shape=(2, max(n, 1)), m=2,
                                n=n, k=k, expect=bad) == bad
    for k in (96, 4160):
        for form in (0, 1):
            assert R.run_int8_stage(R.QUANT_ROWS, form, [z(2, k)], q_shape=(2, k), m=2, k=k, expect=bad) == bad
    # hidden 96 and hidden 1088; a token id past the vocabulary
    for hidden in (96, 1088):
        assert R.run_int8_stage(R.ADD_LN_QUANT, 0, [z(2, hidden), z(2, hidden), z(hidden), z(hidden)], f32_shape=(2, hidden),
                                q_shape=(2, hidden), m=2, hidden=hidden, eps=1e-12, expect=bad) == bad
        assert R.run_int8_stage(R.EMBED_LN_QUANT, 0, [z(4, hidden), z(4, hidden), z(hidden), z(hidden), z(hidden)], ids=[0, 1], positions=[0, 1],
                                f32_shape=(2, hidden), q_shape=(2, hidden), m=2, hidden=hidden, vocab=4, max_pos=4, eps=1e-12, expect=bad) == bad
        assert R.run_head(z(2, hidden), z(hidden, hidden), z(hidden), z(hidden), z(1), expect=bad) == bad
    assert R.run_int8_stage(R.EMBED_LN_QUANT, 0, [z(4, 64), z(4, 64), z(64), z(64), z(64)], ids=[0, 4], positions=[0, 1], f32_shape=(2, 64),
                            q_shape=(2, 64), m=2, hidden=64, vocab=4, max_pos=4, eps=1e-12, expect=bad) == bad
    # unknown stage, form, epilogue; m = 0
    assert R.run_int8_stage(5, 0, [z(2, 64)], q_shape=(2, 64), m=2, k=64, expect=bad) == bad
    assert R.run_int8_stage(R.QUANT_ROWS, 2, [z(2, 64)], q_shape=(2, 64), m=2, k=64, expect=bad) == bad
    assert R.run_int8_stage(R.PACK_W, 1, [z(64, 64)], q_shape=(4096,), n=64, k=64, expect=bad) == bad
    assert R.run_int8_stage(R.GEMM, 0, [z(2), z(64, 64), z(64)], codes=np.zeros((2, 64), np.int8), f32_shape=(2, 64), m=2, n=64, k=64, epilogue=2,
                            expect=bad) == bad
    assert R.run_int8_stage(R.QUANT_ROWS, 0, [z(2, 64)], q_shape=(2, 64), m=0, k=64, expect=bad) == bad
    # null pointers: an input, the codes of the GEMM, an output
    assert R.run_int8_stage(R.QUANT_ROWS, 0, [], q_shape=(2, 64), m=2, k=64, expect=null) == null
    assert R.run_int8_stage(R.GEMM, 0, [z(2), z(64, 64), z(64)], f32_shape=(2, 64), m=2, n=64, k=64, expect=null) == null
    assert R.run_int8_stage(R.QUANT_ROWS, 0, [z(2, 64)], m=2, k=64, expect=null) == null
    assert R.run_int8_stage(R.ADD_LN_QUANT, 0, [z(2, 64), z(2, 64), z(64), z(64)], f32_shape=(2, 64), m=2, hidden=64, expect=null) == null
    assert E.run_stage(R.CLS_HEAD, 0, [z(2, 64), z(64, 64), z(64), z(64)], [(2,), (2,)], m=2, hidden=64, expect=null) == null
    from frankensearch_amd import _lib
    assert _lib.lib().fsgpu_lab_bert_int8_stage(0, None) == null


# ---- the references against the f32 oracles -----------------------------------------------------------------------------------------------

def test_references_agree_with_the_f32_oracles():
    from oracle import bert_oracle as O
    import reranker_ref as RR
    x = np.linspace(-12, 12, 4801)
    assert np.max(np.abs(E.gelu(x) - O.gelu(x.astype(F)))) < 2e-6
    xr, delta, g, beta = R.add_ln_inputs(9, 128, 2)
    out, _ = R.add_ln(xr[2:], delta[2:], g, beta)   # (the row of standard deviation 1e-3 amplifies the oracle's own f32 rounding of the sum: left out)
    assert np.max(np.abs(out - O.layer_norm((xr[2:] + delta[2:]).astype(F), g, beta))) < 1e-5
    ids, positions, word, pos, type0, g, beta = R.embed_inputs(9, 128, 4)
    out, _ = R.embed_ln(ids, positions, word, pos, type0, g, beta)
    want = O.layer_norm(((word[ids] + pos[positions]) + type0).astype(F), g, beta)
    assert np.max(np.abs(out[1:] - want[1:]) / (1 + np.abs(want[1:]))) < 1e-4
    # pooler and classifier as reranker_ref.logits / scores_of state them
    hw = RR.head_weights(3, 128)
    cls = np.random.default_rng(1).standard_normal((7, 128)).astype(F)
    logit, _, score, _ = R.cls_head(cls, hw["bert.pooler.dense.weight"], hw["bert.pooler.dense.bias"], hw["classifier.weight"], hw["classifier.bias"])
    pooled = np.tanh((cls @ hw["bert.pooler.dense.weight"].T + hw["bert.pooler.dense.bias"]).astype(F)).astype(F)
    want = (pooled @ hw["classifier.weight"].reshape(1, -1).T).reshape(-1).astype(F) + hw["classifier.bias"][0]
    assert np.max(np.abs(logit - want)) < 1e-5
    assert np.max(np.abs(score - RR.scores_of(want))) < 1e-6
    # the int8 GEMM's reference is the restatement's linear once the codes are the restatement's own
    xa = np.random.default_rng(2).standard_normal((5, 128)).astype(F)
    w = R.pack_inputs(192, 128, 3)
    b = np.arange(192, dtype=F)
    q, s = Q.quantize_rows(xa)
    assert np.array_equal(R.bits(R.gemm_exact(q, s, w, b)), R.bits(Q.linear_int8_dynamic(xa, w, b)))


# ---- the exact restatements by hand -----------------------------------------------------------------------------------------------------------

def test_exact_restatements_give_hand_computed_answers():
    q, s = Q.quantize_rows(Q.rust_quant_pin_matrix())
    assert q[0].tolist() == [127, 1, -1, 2, -2, 3, -3, 0] and s[0] == 1.0 and not q[1].any() and s[1] == 0.0
    # the tiny-amax rule: a zero is 0 in every row, every other element of a row whose 127 / amax overflows is +-127
    q, s = Q.quantize_rows(F([[1e-38, 0.0, -1e-38, 0.0], [1e-42, 0.0, -3e-45, 1e-45], [3.8e-37, 1e-38, 0.0, -1e-45]]))
    assert q.tolist() == [[127, 0, -127, 0], [127, 0, -127, 127], [127, 3, 0, 0]]
    assert s[0] == F(1e-38) / F(127.0) and s[0] > 0
    # one tile of PACK_W by hand: W [16, 64] with w[n, k] = the code itself on a row of amax 127 (inv = 1), so the packed bytes are w;
    # lane l holds row l & 15, columns 16 (l >> 4) .. + 15
    w = np.zeros((64, 64), F)
    w[:16] = ((np.arange(16)[:, None] * 7 + np.arange(64)[None, :] * 3) % 120).astype(F)
    w[:16, 63] = 127.0
    packed, sw = R.pack_w(w)
    assert np.all(sw[:16] == 1.0) and packed.size == 4096
    tile = packed[:1024].reshape(64, 16)
    for lane in (0, 1, 15, 16, 17, 47, 63):
        assert tile[lane].tolist() == w[lane & 15, 16 * (lane >> 4):16 * (lane >> 4) + 16].astype(int).tolist(), lane
    assert tile[5][3] == (5 * 7 + 3 * 3) % 120 and tile[16 + 5][0] == (5 * 7 + 16 * 3) % 120 and tile[63][15] == 127
    # two k tiles: code (n, k) of a [64, 128] weight lies at tile (n >> 4) * 2 + (k >> 6)
    idx = R.pack_index(64, 128)
    assert idx[0, 0] == 0 and idx[0, 64] == 1024 and idx[16, 0] == 2048 and idx[17, 64 + 16 + 2] == (3 * 64 + 1 + 16) * 16 + 2
    assert sorted(idx.ravel().tolist()) == list(range(64 * 128))
    # the bias epilogue: one accumulator above 2^24 by hand.  127 x 127 x 4096 - 127 = 66,064,257 lies between multiples of 4
    codes = np.full((1, 4096), 127, np.int8)
    codes[0, 0] = 126
    y = R.gemm_exact(codes, F([0.5]), np.full((64, 4096), 0.25, F), np.zeros(64, F))
    assert y[0, 0] == F(66064256.0) * (F(0.5) * (F(0.25) / F(127.0)))


# ---- the comparator is not blind ----------------------------------------------------------------------------------------------------------------

def round_half_even_rows(x):
    """Mutation: quantize_rows with numpy's round (ties to even)."""
    x = np.asarray(x, F)
    amax = np.max(np.abs(x), axis=1)
    inv = np.where(amax > 0, F(127.0) / np.where(amax > 0, amax, F(1.0)), F(0.0)).astype(F)
    return np.clip(np.round((x * inv[:, None]).astype(F)), -127, 127).astype(np.int8)


def test_quantiser_checks_see():
    differs = 0
    for k in R.QUANT_KS:
        for rows in R.QUANT_ROW_COUNTS:
            for family in ("ties", "rust_pin"):
                x = R.quant_inputs(family, rows, k, 100 * k + rows)
                q, _ = Q.quantize_rows(x)
                assert not np.array_equal(round_half_even_rows(x), q), (family, rows, k)
                differs += 1
    assert differs
    # a scale from the neighbouring row; codes quantised from the row before the LayerNorm
    for hidden in R.LN_HIDDEN:
        for tokens in R.LN_TOKENS[1:]:
            x, delta, g, beta = R.add_ln_inputs(tokens, hidden, 11 * hidden + tokens)
            out = R.add_ln(x, delta, g, beta)[0].astype(F)    # stands in for the row the kernel stored
            q, s = Q.quantize_rows(out)
            assert not np.array_equal(R.bits(np.roll(s, 1)), R.bits(s))
            stale_q, stale_s = Q.quantize_rows((x + delta).astype(F))
            assert not np.array_equal(stale_q, q) and not np.array_equal(R.bits(stale_s), R.bits(s))


def test_pack_w_check_sees_a_swapped_fragment_order():
    def swapped(n_rows, k_cols):
        n = np.arange(n_rows)[:, None]
        k = np.arange(k_cols)[None, :]
        tile = (n >> 4) * (k_cols >> 6) + (k >> 6)
        return (tile * 64 + (k & 15) + 16 * ((k & 63) >> 4)) * 16 + (n & 15)     # lane and byte exchanged
    for n, k in R.PACK_SHAPES:
        w = R.pack_inputs(n, k, n + k)
        assert not np.array_equal(R.pack_w(w, swapped)[0], R.pack_w(w)[0]), (n, k)


def gemm_mutated(codes, sa, w, bias, mutation):
    qw, sw = Q.quantize_rows(w)
    acc = Q.int_matmul(codes, qw)
    scale = (sa[:, None] * sw[None, :]).astype(F) if mutation != "sw_alone" else np.repeat(sw[None, :], len(sa), axis=0)
    if mutation == "truncated":
        a = acc.astype(F)
        over = np.abs(a.astype(np.int64)) > np.abs(acc)      # rounded away from zero: step back towards it
        a = np.where(over, np.nextafter(a, F(0.0)), a).astype(F)
    else:
        a = acc.astype(F)
    return ((a * scale).astype(F) + bias[None, :]).astype(F)


def test_gemm_checks_see():
    for m, n, k in [(1, 192, 128), (33, 64, 64), (65, 384, 1536)]:
        codes, sa, w, bias = R.gemm_inputs("random", m, n, k, 7 * m + 3 * n + k)
        want = R.gemm_exact(codes, sa, w, bias)
        assert np.array_equal(R.bits(gemm_mutated(codes, sa, w, bias, "none")), R.bits(want))
        assert not np.array_equal(R.bits(gemm_mutated(codes, sa, w, bias, "sw_alone")), R.bits(want))
    for m, n in [(1, 64), (33, 192)]:
        codes, sa, w, bias = R.gemm_inputs("extreme_odd", m, n, 4096, 7 * m + 3 * n + 4096)
        want = R.gemm_exact(codes, sa, w, bias)
        assert not np.array_equal(R.bits(gemm_mutated(codes, sa, w, bias, "truncated")), R.bits(want)), (m, n)


def gelu_tanh(x):
    return 0.5 * x * (1.0 + np.tanh(np.sqrt(2.0 / np.pi) * (x + 0.044715 * x ** 3)))


def gelu_f32(x):
    """The 7.1.26 form evaluated in f32 numpy, as the kernel states it."""
    x = np.asarray(x, F)
    z = (x * F(0.70710678118654752440)).astype(F)
    t = (F(1.0) / (F(1.0) + F(0.3275911) * np.abs(z))).astype(F)
    poly = t * (F(0.2548296) + t * (F(-0.28449673) + t * (F(1.4214137) + t * (F(-1.453152) + t * F(1.0614054)))))
    erf = np.copysign(F(1.0) - poly * np.exp(-(z * z)), z).astype(F)
    return (F(0.5) * x * (F(1.0) + erf)).astype(F)


@pytest.mark.parametrize("family,m,n,k", [("gelu_sweep", 33, 192, 64), ("random", 33, 192, 128), ("random", 65, 384, 1536)])
def test_gelu_check_sees_and_the_reference_sits_inside_its_bound(family, m, n, k):
    codes, sa, w, bias = R.gemm_inputs(family, m, n, k, 7 * m + 3 * n + k)
    pre = R.gemm_exact(codes, sa, w, bias)
    ref, bound = R.gemm_gelu(codes, sa, w, bias)
    factor = R.SAFETY["gemm_gelu"]
    assert E.compare(gelu_f32(pre), ref, bound) <= 1.0
    assert E.compare(gelu_tanh(pre.astype(np.float64)), ref, bound * factor) >= BLIND
    assert E.compare(pre, ref, bound * factor) >= BLIND             # GELU skipped


def layer_norm_f32(y, g, beta, eps=R.LN_EPS):
    y = np.asarray(y, F)
    mean = (y.sum(axis=-1, keepdims=True, dtype=F) / F(y.shape[-1])).astype(F)
    d = (y - mean).astype(F)
    var = ((d * d).sum(axis=-1, keepdims=True, dtype=F) / F(y.shape[-1])).astype(F)
    inv = (F(1.0) / np.sqrt((var + F(eps)).astype(F))).astype(F)
    return ((d * inv).astype(F) * g + beta).astype(F)


@pytest.mark.parametrize("hidden", R.LN_HIDDEN)
def test_layer_norm_checks_see_and_the_references_sit_inside_their_bounds(hidden):
    for tokens in R.LN_TOKENS:
        x, delta, g, beta = R.add_ln_inputs(tokens, hidden, 11 * hidden + tokens)
        ref, bound = R.add_ln(x, delta, g, beta)
        assert E.compare(layer_norm_f32((x + delta).astype(F), g, beta), ref, bound) <= 1.0, (hidden, tokens)
        factor = R.SAFETY["add_ln_quant"]
        unbiased = beta + (ref - beta) * np.sqrt((hidden - 1) / hidden)       # variance divided by H - 1
        assert E.compare(unbiased, ref, bound * factor) >= BLIND
        if tokens > 1:
            assert E.compare(np.roll(ref, 1, axis=0), ref, bound * factor) >= BLIND   # a stale row
        ids, positions, word, pos, type0, g, beta = R.embed_inputs(tokens, hidden, 7 * hidden + tokens)
        ref, bound = R.embed_ln(ids, positions, word, pos, type0, g, beta)
        v = ((word[ids] + pos[positions]).astype(F) + type0).astype(F)
        assert E.compare(layer_norm_f32(v, g, beta), ref, bound) <= 1.0, (hidden, tokens)
        factor = R.SAFETY["embed_ln_quant"]
        if tokens > 1:   # (the one-token call is the row at a mean of 50, whose bound is the widest)
            assert E.compare(beta + (ref - beta) * np.sqrt((hidden - 1) / hidden), ref, bound * factor) >= BLIND


def head_f32(x, pool_w, pool_b, w_c, b_c):
    pre = ((x @ pool_w.T).astype(F) + pool_b).astype(F)
    pooled = np.tanh(pre).astype(F)
    logit = ((pooled @ w_c).astype(F) + b_c[0]).astype(F)
    with np.errstate(over="ignore"):
        score = (F(1.0) / (F(1.0) + np.exp(-logit).astype(F))).astype(F)
    return logit, score


def test_head_checks_see_and_the_reference_sits_inside_its_bound():
    """The mutations must reach the ratio at every width, on one of the calls the GPU test makes at that width at least (a single pair
    whose logit happens to lie near 0 shows neither a missing tanh nor a flipped sign)."""
    factor = R.SAFETY["cls_head"]
    for hidden in R.HEAD_HIDDEN:
        seen = {"no_tanh": 0.0, "minus_logit": 0.0}
        for pairs in R.HEAD_PAIRS:
            seed = 3 * hidden + pairs
            cases = [R.head_inputs("ordinary", pairs, hidden, seed), R.head_inputs("saturated", pairs, hidden, seed)]
            cases += [R.head_inputs("extreme", pairs, hidden, seed, b) for b in R.HEAD_BIASES]
            for i, ins in enumerate(cases):
                logit, dlogit, score, dscore = R.cls_head(*ins)
                got_logit, got_score = head_f32(*ins)
                assert E.compare(got_logit, logit, dlogit) <= 1.0 and E.compare(got_score, score, dscore) <= 1.0, (hidden, pairs, i)
                if i < 2:
                    seen["no_tanh"] = max(seen["no_tanh"], E.compare(R.cls_head(*ins, tanh=lambda v: v)[0], logit, dlogit * factor))
                    seen["minus_logit"] = max(seen["minus_logit"], E.compare(R.cls_head(*ins, sign=-1.0)[2], score, dscore * factor))
                else:
                    # beyond +-90 the sign is the whole answer
                    assert E.compare(R.cls_head(*ins, sign=-1.0)[2], score, dscore * factor) >= BLIND
        assert min(seen.values()) >= BLIND, (hidden, seen)

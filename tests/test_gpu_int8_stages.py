"""The int8 encoder's kernels launch by launch, through fsgpu_lab_bert_int8_stage (the product's own launch_bert_i8_* functions on host
arrays), and the cross-encoder's head through the CLS_HEAD stage of fsgpu_lab_bert_stage, against tests/int8_stage_ref.py: quantiser
codes and scales, packed weight bytes and the bias-epilogue GEMM bit for bit; the GELU epilogue, the f32 rows of the two
LayerNorm-quantisers and the head inside derived bounds (ratio <= SAFETY[stage]).  Then the product's forward_int8 as the composition of
those launches: the chain run from Python, one lab call per launch, gives the embedder's vectors bit for bit."""
import functools
import os

import numpy as np
import pytest

import encoder_stage_ref as E
import int8_dynamic_ref as Q
import int8_stage_ref as R

pytestmark = pytest.mark.gpu
RATIOS = {}   # (stage, form) -> (largest ratio seen in this run, factor)


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    build()
    yield
    path = os.environ.get("FSGPU_STAGE_RATIOS")   # (how profiles/int8_stages/ratios.txt is made)
    if path:
        with open(path, "a") as f:
            for (stage, form), (ratio, safety) in sorted(RATIOS.items(), key=str):
                f.write(f"{stage:15s} form {str(form):28s} max ratio {ratio:.4f}  safety {safety:g}\n")


def check(stage, form, got, ref, bound, what, safety=None):
    ratio = E.compare(got, ref, bound)
    safety = R.SAFETY[stage] if safety is None else safety
    RATIOS[(stage, form)] = (max(RATIOS.get((stage, form), (0.0, 0.0))[0], ratio), safety)
    print(f"{stage} form {form} {what}: ratio {ratio:.4f}")
    assert ratio <= safety, f"{stage} form {form} {what}: ratio {ratio:.3f}"


def same_bits(got, want, what):
    got, want = R.bits(got), R.bits(want)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int(np.sum(got != want)), np.argwhere(got != want)[:4].tolist())


def check_quantised(out, x, what):
    """Codes and scales are the quantisation of the f32 rows x, bit for bit."""
    q, s = Q.quantize_rows(x)
    same_bits(out["q"], q, what + ": codes")
    same_bits(out["s"], s, what + ": scales")


# ---- the row quantiser --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", R.QUANT_KS)
@pytest.mark.parametrize("form", [0, 1])
def test_quant_rows(form, k):
    """Four rows make a block: 1, 3, 4, 5 and 33 rows.  Form 1 quantises the f16 rounding of its input (the attention context)."""
    for rows in R.QUANT_ROW_COUNTS:
        for family in (R.QUANT_FAMILIES_F16 if form else R.QUANT_FAMILIES):
            x = R.quant_inputs(family, rows, k, 100 * k + rows)
            out = R.run_int8_stage(R.QUANT_ROWS, form, [x], q_shape=(rows, k), m=rows, k=k)
            check_quantised(out, E.h16(x) if form else x, f"form {form} {family} rows {rows} k {k}")


def test_quant_rows_tiny_amax_contract():
    """0 < amax < 127 / FLT_MAX: 127 / amax is +inf.  A zero codes to 0, every other element to +-127; the scale is amax / 127."""
    k = 64
    x = np.zeros((5, k), np.float32)
    x[0, :4] = [1e-38, 0.0, -1e-38, 0.0]
    x[1, :4] = [1e-42, 0.0, -3e-45, 1e-45]            # subnormal amax
    x[2, :4] = [3.7e-37, -1e-45, 0.0, 1e-40]          # just below the threshold
    x[3, :4] = [3.8e-37, 1e-38, 0.0, -1e-45]          # just above it: 127 / amax is finite, ordinary rounding
    x[4, k - 1] = -2e-38
    out = R.run_int8_stage(R.QUANT_ROWS, 0, [x], q_shape=(5, k), m=5, k=k)
    q = out["q"]
    assert q[0, :4].tolist() == [127, 0, -127, 0] and q[1, :4].tolist() == [127, 0, -127, 127]
    assert q[2, :4].tolist() == [127, -127, 0, 127] and q[3, :4].tolist() == [127, 3, 0, 0]
    assert q[4, k - 1] == -127 and not q[:, 4:k - 1].any()
    check_quantised(out, x, "tiny amax")
    # the weight packer shares the rule
    w = np.zeros((64, k), np.float32)
    w[:5] = x
    out = R.run_pack(w)
    packed, sw = R.pack_w(w)
    same_bits(out["q"], packed, "tiny amax packed")
    same_bits(out["s"], sw, "tiny amax sw")


# ---- the weight packer ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n,k", R.PACK_SHAPES)
def test_pack_w(n, k):
    w = R.pack_inputs(n, k, n + k)
    out = R.run_pack(w)
    packed, sw = R.pack_w(w)
    same_bits(out["q"], packed, f"pack_w {n} x {k}: bytes")
    same_bits(out["s"], sw, f"pack_w {n} x {k}: scales")
    assert not sw[3] and sw[5] == np.float32(0.3) / np.float32(127.0)


# ---- the GEMM -----------------------------------------------------------------------------------------------------------------------------------

def run_gemm(family, m, n, k, epilogue, seed=None):
    codes, sa, w, bias = R.gemm_inputs(family, m, n, k, 7 * m + 3 * n + k if seed is None else seed)
    y = R.run_int8_stage(R.GEMM, 0, [sa, w, bias], codes=codes, f32_shape=(m, n), m=m, n=n, k=k, epilogue=epilogue)["x"]
    what = f"{family} m {m} n {n} k {k}"
    if epilogue == 0:
        same_bits(y, R.gemm_exact(codes, sa, w, bias), what)
    else:
        ref, bound = R.gemm_gelu(codes, sa, w, bias)
        check("gemm_gelu", family, y, ref, bound, what)
    return y, (codes, sa, w, bias)


@pytest.mark.parametrize("epilogue", [0, 1])
def test_gemm_shapes(epilogue):
    """The 16-row fragment, 32-row wave and 64-row block edges with the clamped reads past M; N = 64 and 192 leave the block's second
    wave column empty."""
    for m, n, k in R.gemm_shapes():
        run_gemm("random", m, n, k, epilogue)


@pytest.mark.parametrize("epilogue", [0, 1])
def test_gemm_zero_scales_and_cancelling_sums(epilogue):
    for m, n, k in [(1, 192, 128), (33, 192, 128), (65, 192, 128), (33, 384, 1536), (65, 64, 64)]:
        y, (_, _, _, bias) = run_gemm("sa_zero", m, n, k, epilogue)
        if epilogue == 0:
            assert np.array_equal(y[0], bias) and np.array_equal(y[-1], bias)
        y, (_, _, _, bias) = run_gemm("cancel", m, n, k, epilogue)
        if epilogue == 0:
            assert np.array_equal(y, np.repeat(bias[None, :], m, axis=0))


@pytest.mark.parametrize("epilogue", [0, 1])
def test_gemm_accumulators_above_2_pow_24(epilogue):
    """K = 4096 with every code at +-127: |acc| = 66,064,384; with a few codes at 126 the accumulators take every residue and
    (float)acc rounds."""
    for m, n in [(1, 64), (33, 192), (65, 192)]:
        _, (codes, _, w, _) = run_gemm("extreme", m, n, 4096, epilogue)
        acc = Q.int_matmul(codes, Q.quantize_rows(w)[0])
        assert np.all(np.abs(acc) == 66064384)
        _, (codes, _, w, _) = run_gemm("extreme_odd", m, n, 4096, epilogue)
        acc = Q.int_matmul(codes, Q.quantize_rows(w)[0])
        assert np.all(np.abs(acc) > 2 ** 24) and np.any(acc.astype(np.float32).astype(np.int64) != acc)


def test_gemm_gelu_over_the_whole_erf_range():
    """Zero codes: the pre-activation is the bias, which sweeps [-12, 12] (the negative tail, where 1 + erf cancels) with +0 and -0."""
    for m in (1, 33):
        y, (_, _, _, bias) = run_gemm("gelu_sweep", m, 192, 64, 1)
        assert np.all(y[:, -2:] == 0) and np.all(y[:, bias > 6] == bias[bias > 6])
        same = run_gemm("gelu_sweep", m, 192, 64, 0)[0]
        assert np.array_equal(same, np.repeat(bias[None, :], m, axis=0))


# ---- embedding / residual + LayerNorm + quantise ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", R.LN_HIDDEN)
def test_embed_ln_quant(hidden):
    for tokens in R.LN_TOKENS:
        ids, positions, word, pos, type0, g, beta = R.embed_inputs(tokens, hidden, 7 * hidden + tokens)
        out = R.run_int8_stage(R.EMBED_LN_QUANT, 0, [word, pos, type0, g, beta], ids=ids, positions=positions, f32_shape=(tokens, hidden),
                               q_shape=(tokens, hidden), m=tokens, hidden=hidden, vocab=word.shape[0], max_pos=pos.shape[0], eps=R.LN_EPS)
        what = f"hidden {hidden} tokens {tokens}"
        ref, bound = R.embed_ln(ids, positions, word, pos, type0, g, beta)
        check("embed_ln_quant", 0, out["x"], ref, bound, what)
        check_quantised(out, out["x"], what)


@pytest.mark.parametrize("hidden", R.LN_HIDDEN)
def test_add_ln_quant(hidden):
    """Form 1 (q = NULL, the last layer's call) returns the x bits of form 0 and leaves the code and scale buffers alone (the lab
    entry fails with "guard band" otherwise)."""
    for tokens in R.LN_TOKENS:
        x, delta, g, beta = R.add_ln_inputs(tokens, hidden, 11 * hidden + tokens)
        kw = dict(f32_shape=(tokens, hidden), m=tokens, hidden=hidden, eps=R.LN_EPS)
        out = R.run_int8_stage(R.ADD_LN_QUANT, 0, [x, delta, g, beta], q_shape=(tokens, hidden), **kw)
        what = f"hidden {hidden} tokens {tokens}"
        ref, bound = R.add_ln(x, delta, g, beta)
        check("add_ln_quant", 0, out["x"], ref, bound, what)
        check_quantised(out, out["x"], what)
        bare = R.run_int8_stage(R.ADD_LN_QUANT, 1, [x, delta, g, beta], **kw)
        same_bits(bare["x"], out["x"], what + ": form 1")


# ---- the product is the composition -------------------------------------------------------------------------------------------------------------

LENGTHS = [1, 5, 33, 0, 64]


@pytest.mark.parametrize("hidden,inter", [(128, 256), (384, 1536)])
@pytest.mark.parametrize("layers", [1, 2])
def test_forward_int8_is_the_composition_of_its_launches(layers, hidden, inter):
    """NativeEmbedder::forward_int8 launch by launch from Python, every intermediate through the host, every launch against its reference
    on the operands the GPU itself produced; the final vectors equal the embedder's bit for bit — which also covers the reuse of its
    code, scale and scratch buffers and the q = NULL of the last layer."""
    import frankensearch_amd as fa
    from oracle import bert_oracle
    vocab = 200
    w = bert_oracle.random_weights(40 + layers, vocab, hidden, layers, inter)
    rng = np.random.default_rng(hidden + layers)
    batch = [rng.integers(0, vocab, n).tolist() for n in LENGTHS]
    offsets = E.offsets_of(LENGTHS)
    t = int(offsets[-1])
    ids = np.concatenate([np.asarray(b, np.int32) for b in batch if b])
    positions = np.concatenate([np.arange(n, dtype=np.int32) for n in LENGTHS if n])
    what = f"hidden {hidden} inter {inter} layers {layers}"

    def gemm(q, s, weight, bias, epilogue, tag):
        n, k = weight.shape
        y = R.run_int8_stage(R.GEMM, 0, [s, weight, bias], codes=q, f32_shape=(t, n), m=t, n=n, k=k, epilogue=epilogue)["x"]
        if epilogue == 0:
            same_bits(y, R.gemm_exact(q, s, weight, bias), f"{what} {tag}")
        else:
            check("gemm_gelu", "chain", y, *R.gemm_gelu(q, s, weight, bias), f"{what} {tag}")
        return y

    word, pos = w["embeddings.word_embeddings.weight"], w["embeddings.position_embeddings.weight"]
    type0 = w["embeddings.token_type_embeddings.weight"][0]
    g, beta = w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"]
    out = R.run_int8_stage(R.EMBED_LN_QUANT, 0, [word, pos, type0, g, beta], ids=ids, positions=positions, f32_shape=(t, hidden),
                           q_shape=(t, hidden), m=t, hidden=hidden, vocab=vocab, max_pos=pos.shape[0], eps=R.LN_EPS)
    check("embed_ln_quant", "chain", out["x"], *R.embed_ln(ids, positions, word, pos, type0, g, beta), what)
    check_quantised(out, out["x"], what + " embed")
    x, q, s = out["x"], out["q"], out["s"]
    for layer in range(layers):
        p = f"encoder.layer.{layer}"
        last = layer == layers - 1
        wqkv = np.concatenate([w[f"{p}.attention.self.{n}.weight"] for n in ("query", "key", "value")], axis=0)
        bqkv = np.concatenate([w[f"{p}.attention.self.{n}.bias"] for n in ("query", "key", "value")], axis=0)
        qkv = gemm(q, s, wqkv, bqkv, 0, f"layer {layer} qkv")
        ctx, = E.run_stage(E.ATTENTION, 1, [qkv], [(t, hidden)], offsets=offsets, m=t, hidden=hidden, n_docs=len(LENGTHS), scale=E.ATTN_SCALE)
        ref, bound = E.attention(E.h16(qkv), offsets, hidden)   # (bert_attention_mfma_kernel<float> rounds Q, K, V to f16 as it loads them)
        assert E.compare(ctx, ref, bound) <= E.SAFETY["attention"], f"{what} layer {layer} attention"
        out = R.run_int8_stage(R.QUANT_ROWS, 1, [ctx], q_shape=(t, hidden), m=t, k=hidden)
        check_quantised(out, ctx, f"{what} layer {layer} ctx")
        tmp = gemm(out["q"], out["s"], w[f"{p}.attention.output.dense.weight"], w[f"{p}.attention.output.dense.bias"], 0, f"layer {layer} ao")
        g, beta = w[f"{p}.attention.output.LayerNorm.weight"], w[f"{p}.attention.output.LayerNorm.bias"]
        out = R.run_int8_stage(R.ADD_LN_QUANT, 0, [x, tmp, g, beta], f32_shape=(t, hidden), q_shape=(t, hidden), m=t, hidden=hidden, eps=R.LN_EPS)
        check("add_ln_quant", "chain", out["x"], *R.add_ln(x, tmp, g, beta), f"{what} layer {layer} ln1")
        check_quantised(out, out["x"], f"{what} layer {layer} ln1")
        x = out["x"]
        mid = gemm(out["q"], out["s"], w[f"{p}.intermediate.dense.weight"], w[f"{p}.intermediate.dense.bias"], 1, f"layer {layer} ffn-in")
        out = R.run_int8_stage(R.QUANT_ROWS, 0, [mid], q_shape=(t, inter), m=t, k=inter)
        check_quantised(out, mid, f"{what} layer {layer} gelu")
        tmp = gemm(out["q"], out["s"], w[f"{p}.output.dense.weight"], w[f"{p}.output.dense.bias"], 0, f"layer {layer} ffn-out")
        g, beta = w[f"{p}.output.LayerNorm.weight"], w[f"{p}.output.LayerNorm.bias"]
        out = R.run_int8_stage(R.ADD_LN_QUANT, 1 if last else 0, [x, tmp, g, beta], f32_shape=(t, hidden),
                               q_shape=None if last else (t, hidden), m=t, hidden=hidden, eps=R.LN_EPS)
        check("add_ln_quant", "chain", out["x"], *R.add_ln(x, tmp, g, beta), f"{what} layer {layer} ln2")
        x = out["x"]
        if not last:
            check_quantised(out, x, f"{what} layer {layer} ln2")
            q, s = out["q"], out["s"]
    pooled, = E.run_stage(E.POOL, 0, [x], [(len(LENGTHS), hidden)], offsets=offsets, m=t, hidden=hidden, n_docs=len(LENGTHS))
    ref, bound = E.pool(x, offsets)
    assert E.compare(pooled, ref, bound) <= E.SAFETY["pool"], what + " pool"
    product = fa.NativeEmbedder(w, linear="int8_dynamic").embed_batch_token_ids(batch)
    same_bits(pooled, product, what + ": the embedder's vectors")
    assert np.all(product[3] == 0)


# ---- the cross-encoder's head -----------------------------------------------------------------------------------------------------------------------

def check_head(ins, what, form):
    logits, scores = R.run_head(*ins)
    logit, dlogit, score, dscore = R.cls_head(*ins)
    check("cls_head", f"{form} logit", logits, logit, dlogit, what)
    check("cls_head", f"{form} score", scores, score, dscore, what)
    return logits, scores


@pytest.mark.parametrize("hidden", R.HEAD_HIDDEN)
def test_cls_head(hidden):
    for pairs in R.HEAD_PAIRS:
        seed = 3 * hidden + pairs
        check_head(R.head_inputs("ordinary", pairs, hidden, seed), f"hidden {hidden} pairs {pairs}", "ordinary")
        ins = R.head_inputs("saturated", pairs, hidden, seed)
        assert np.max(np.abs(ins[0].astype(np.float64) @ ins[1].astype(np.float64).T)) > 20
        check_head(ins, f"hidden {hidden} pairs {pairs}", "saturated")
        for b in R.HEAD_BIASES:
            logits, scores = check_head(R.head_inputs("extreme", pairs, hidden, seed, b), f"hidden {hidden} pairs {pairs} bias {b}", "extreme")
            assert np.all(np.abs(logits) > 89.5)
            assert np.all(scores == (1.0 if b > 0 else 0.0)), (b, scores)   # exp(-logit) underflows against 1 / overflows to +inf


@pytest.mark.parametrize("hidden", R.HEAD_HIDDEN)
def test_cls_head_non_finite_pair(hidden):
    """A NaN and an Inf in ONE pair's [CLS] row: that pair scores 0.0 with a non-finite logit; every other pair keeps the bits it has
    when it is scored alone."""
    for pairs in R.HEAD_PAIRS:
        x, pool_w, pool_b, w_c, b_c = R.head_inputs("ordinary", pairs, hidden, 5 * hidden + pairs)
        bad = pairs // 2
        x[bad, 5] = np.nan
        x[bad, hidden - 3] = np.inf
        logits, scores = R.run_head(x, pool_w, pool_b, w_c, b_c)
        assert not np.isfinite(logits[bad]) and scores[bad] == 0.0 and not np.signbit(scores[bad])
        for p in range(pairs):
            if p == bad:
                continue
            lone_logit, lone_score = R.run_head(x[p:p + 1], pool_w, pool_b, w_c, b_c)
            same_bits(logits[p:p + 1], lone_logit, f"hidden {hidden} pair {p}")
            same_bits(scores[p:p + 1], lone_score, f"hidden {hidden} pair {p}")
        ok = np.arange(pairs) != bad
        if ok.any():
            logit, dlogit, score, dscore = R.cls_head(x[ok], pool_w, pool_b, w_c, b_c)
            check("cls_head", "beside NaN logit", logits[ok], logit, dlogit, f"hidden {hidden} pairs {pairs}")
            check("cls_head", "beside NaN score", scores[ok], score, dscore, f"hidden {hidden} pairs {pairs}")


def test_cls_head_refuses_unsupported_widths():
    for hidden in (96, 1088):
        ins = R.head_inputs("ordinary", 2, hidden, 1)
        assert R.run_head(*ins, expect=2) == 2

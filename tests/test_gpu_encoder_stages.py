"""The f16 encoder's kernels stage by stage, through fsgpu_lab_bert_stage (the product's own launchers on host arrays), against the f64
references and derived bounds of tests/encoder_stage_ref.py: attention (f16, f32 and [CLS] forms), the linears of every form and
epilogue, linear + residual + LayerNorm, the post-attention block, embedding + LayerNorm and pooling — at the row counts, lengths and
shapes where a launcher changes kernel or a tile ends.  Pass condition: max |got - ref| / bound <= SAFETY[stage] for an f16 output,
<= SAFETY_F32 for an f32 one."""
import functools
import os

import numpy as np
import pytest

import encoder_stage_ref as R

pytestmark = pytest.mark.gpu
RATIOS = {}   # (stage, form) -> largest ratio seen in this run


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    build()
    yield
    path = os.environ.get("FSGPU_STAGE_RATIOS")   # (how profiles/encoder_stages/ratios.txt is made)
    if path:
        with open(path, "a") as f:
            for (stage, form), (ratio, safety) in sorted(RATIOS.items(), key=str):
                f.write(f"{stage:10s} form {str(form):28s} max ratio {ratio:.4f}  safety {safety:g}\n")


def check_repeats(out, what):
    """Rows of a large-M call repeat every UNIQUE_ROWS rows, and a row's arithmetic depends on nothing but the row (a text's
    bits do not depend on what shares its launch): equal inputs, equal bits — whatever tile, block or walker a row fell to."""
    first = out[:R.UNIQUE_ROWS]
    assert np.array_equal(out.view(np.uint32), R.tile_rows(first, out.shape[0]).view(np.uint32)), what + ": repeated rows differ"


def check(stage, form, got, ref, bound, what, f16=True):
    """f16: the output was stored as f16 (the stage's factor); an f32 output is held to the bare bound."""
    ratio = R.compare(got, ref, bound)
    safety = R.SAFETY[stage] if f16 else R.SAFETY_F32
    RATIOS[(stage, form)] = (max(RATIOS.get((stage, form), (0.0, 0.0))[0], ratio), safety)
    assert ratio <= safety, f"{stage} form {form} {what}: ratio {ratio:.3f}"


# ---- attention ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def attention_case(family, lens, hidden, seed, rot, cls):
    """(qkv, offsets, reference, bound): computed once, shared by the forms that take the same operands (0 and 1)."""
    qkv = R.attention_inputs(family, lens, hidden, seed, rot)
    offsets = R.offsets_of(lens)
    ref, bound = R.attention(qkv, offsets, hidden, cls=cls)
    for a in (qkv, offsets, ref, bound):
        a.setflags(write=False)
    return qkv, offsets, ref, bound


def run_attention(form, hidden, family, lens, seed, rot=0):
    cls = form == 2
    qkv, offsets, ref, bound = attention_case(family, tuple(lens), hidden, seed, rot, cls)
    m, n_docs = qkv.shape[0], len(lens)
    scalars = dict(m=m, hidden=hidden, n_docs=n_docs, scale=R.ATTN_SCALE)
    what = f"hidden {hidden} {family} lens {list(lens)[:8]}"
    if cls:
        x = np.random.default_rng(seed).standard_normal((m, hidden)).astype(np.float32)
        ctx, x_cls = R.run_stage(R.ATTENTION, 2, [qkv, x], [(n_docs, hidden), (n_docs, hidden)], offsets=offsets, **scalars)
        assert np.array_equal(x_cls.view(np.uint32), x[offsets[:-1]].view(np.uint32)), what
    else:
        ctx, = R.run_stage(R.ATTENTION, form, [qkv], [(m, hidden)], offsets=offsets, **scalars)
    check("attention", f"{form} {family}", ctx, ref, bound, what)
    if family == "uniform" and not cls:
        # Q = 0: every row of a document is the same mean
        for a, b in zip(offsets[:-1], offsets[1:]):
            assert np.all(ctx[a:b] == ctx[a:a + 1]) or b == a, what


@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
@pytest.mark.parametrize("hidden", [128, 384])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_attention_single_document_lengths(form, hidden, family):
    """One document per call, so max_seq is the length: every 16-query tile and 32-key block edge, the two-block split above 128
    tokens, the LDS request of the f16 form crossing 64 KB between 505 and 512."""
    for i, s in enumerate(R.ATTN_LENGTHS):
        run_attention(form, hidden, family, [s], 1000 + s, rot=i)


@pytest.mark.parametrize("family", R.ATTN_FAMILIES)
@pytest.mark.parametrize("hidden", [128, 384])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_attention_ragged_documents(form, hidden, family):
    for i, lens in enumerate(R.attention_ragged(hidden // 32, cls=form == 2)):
        run_attention(form, hidden, family, lens, 2000 + i)


def test_attention_refuses_what_the_product_never_sends():
    qkv = R.attention_inputs("trained", [4, 0], 128, 1)
    x = np.zeros((4, 128), np.float32)
    kw = dict(m=4, hidden=128, n_docs=2, scale=R.ATTN_SCALE, expect=2)
    assert R.run_stage(R.ATTENTION, 2, [qkv, x], [(2, 128), (2, 128)], offsets=[0, 4, 4], **kw) == 2        # empty pair
    assert R.run_stage(R.ATTENTION, 0, [qkv], [(4, 128)], offsets=[0, 3, 5], **kw) == 2                     # offsets past m
    big = np.zeros((513, 384), np.float32)
    assert R.run_stage(R.ATTENTION, 0, [big], [(513, 128)], offsets=[0, 513], m=513, hidden=128, n_docs=1, scale=1.0, expect=2) == 2


# ---- linear -----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def linear_case(n, k, epilogue, packed):
    a, w, b = R.linear_inputs(n, k, 31 * n + k)
    ref, bound = R.linear(a, w, b, epilogue, packed)
    return a, w, b, ref, bound


def run_linear(form, m, n, k, epilogue):
    a, w, b, ref, bound = linear_case(n, k, epilogue, form != 0)
    y, = R.run_stage(R.LINEAR, form, [R.tile_rows(a, m), w, b], [(m, n)], m=m, n=n, k=k, epilogue=epilogue)
    if m > R.UNIQUE_ROWS:
        check_repeats(y, f"linear form {form} m {m} n {n} k {k} epilogue {epilogue}")
    check("linear", f"{form} epilogue {epilogue}", y, R.tile_rows(ref, m), R.tile_rows(bound, m), f"m {m} n {n} k {k} epilogue {epilogue}", f16=epilogue != 0)


@pytest.mark.parametrize("n,k", [(1536, 512), (768, 768), (3072, 768), (768, 3072), (384, 2048)])
def test_linear_unpacked(n, k):
    """launch_bert_gemm (the path of hidden > 384 and of inter 2048): the direct-fragment kernel up to 64 rows, the LDS-tiled one above."""
    for epilogue in (0, 1):
        for m in (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 257):
            run_linear(0, m, n, k, epilogue)


@pytest.mark.parametrize("k", [128, 256, 384])
@pytest.mark.parametrize("form", [1, 2])
def test_linear_packed(form, k):
    for n in (3 * k, 4 * k):
        for epilogue in (0, 1, 2):
            for m in (1, 63, 64, 65, 129):
                run_linear(form, m, n, k, epilogue)


@pytest.mark.parametrize("n,k", [(1152, 384), (1536, 384), (768, 256), (384, 128)])
def test_linear_packed_across_the_weight_stationary_switch(n, k):
    """launch_bert_gemm_w from 96 row tiles on: 6080 rows are the last call of the 64-row-tile kernel, 6081 the first of
    bert_gemm_wq_kernel (one row in its last tile), 6145 and 8200 leave other tails and walker counts."""
    for epilogue in (0, 1, 2):
        for m in (6080, 6081, 6145, 8200):
            run_linear(1, m, n, k, epilogue)


def test_linear_refuses_unsupported_shapes():
    a, w, b = np.zeros((2, 512), np.float32), np.zeros((512, 512), np.float32), np.zeros(512, np.float32)
    for form in (1, 2):
        assert R.run_stage(R.LINEAR, form, [a, w, b], [(2, 512)], m=2, n=512, k=512, expect=2) == 2      # K = 512: no packed form
    assert R.run_stage(R.LINEAR, 0, [a, w, b], [(2, 512)], m=2, n=512, k=512, epilogue=2, expect=2) == 2   # no plain-f16 epilogue


# ---- linear + residual + LayerNorm ----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def linear_ln_case(hidden, k):
    ins = R.linear_ln_inputs(hidden, k, 17 * hidden + k)
    return ins, R.linear_ln(*ins)


def check_two_copies(stage, form, outs, refs, m, what):
    x, x_h = outs
    ref, bound, bound_h = (R.tile_rows(r, m) for r in refs)
    assert R.is_rne_f16_of(x_h, x), what
    check(stage, f"{form} f32", x, ref, bound, what, f16=False)
    check(stage, f"{form} f16 copy", x_h, ref, bound_h, what)


LN_SHAPES = [(128, 128), (128, 512), (256, 256), (256, 1024), (384, 384), (384, 1536), (128, 2048)]


@pytest.mark.parametrize("hidden,k", LN_SHAPES + [(512, 512), (1024, 1024), (384, 2048)])
@pytest.mark.parametrize("form", [0, 1, 2])
def test_linear_residual_layer_norm(form, hidden, k):
    """Rows of standard deviation 1e-3 and rows with |mean| >> sigma among ordinary ones; row counts around the 4-row, 32-row tiles.
    hidden 512 / 1024 exist for the unpacked form alone (GEMM + bert_add_ln); (384, 2048) is what inter 2048 sends to bert_gemm_ln."""
    if (hidden, k) not in LN_SHAPES and (form == 1 or (form == 0 and hidden > 384)):
        (a, w, b, x, g, beta), _ = linear_ln_case(hidden, k)
        assert R.run_stage(R.LINEAR_LN, form, [a[:2], w, b, x[:2], g, beta], [(2, hidden)] * 2, m=2, hidden=hidden, k=k, eps=R.LN_EPS,
                           expect=2) == 2
        return
    (a, w, b, x, g, beta), refs = linear_ln_case(hidden, k)
    for m in (1, 3, 4, 5, 31, 32, 33, 65, 300):
        outs = R.run_stage(R.LINEAR_LN, form, [R.tile_rows(a, m), w, b, R.tile_rows(x, m), g, beta], [(m, hidden)] * 2, m=m, hidden=hidden,
                           k=k, eps=R.LN_EPS)
        if m > R.UNIQUE_ROWS:
            check_repeats(outs[0], f"linear_ln form {form} hidden {hidden} k {k} m {m}")
        check_two_copies("linear_ln", form, outs, refs, m, f"hidden {hidden} k {k} m {m}")


# ---- post-attention block -----------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def post_attn_case(hidden, inter):
    ins = R.post_attn_inputs(hidden, inter, 13 * hidden + inter)
    return ins, R.post_attn(*ins)


def run_post_attn(form, hidden, inter, m):
    ins, refs = post_attn_case(hidden, inter)
    tiled = [R.tile_rows(ins[0], m)] + list(ins[1:11]) + [R.tile_rows(ins[11], m)]
    outs = R.run_stage(R.POST_ATTN, form, tiled, [(m, hidden)] * 2, m=m, hidden=hidden, inter=inter, eps=R.LN_EPS)
    what = f"hidden {hidden} inter {inter} m {m}"
    if m > R.UNIQUE_ROWS:
        check_repeats(outs[0], what)
    check_two_copies("post_attn", form, outs, refs[:3], m, what)
    # the second LayerNorm's invariant, which no error of the steps before it touches
    tol_mean, tol_m2, m2 = (R.tile_rows(t, m) for t in refs[3])
    mean, second = R.ln_moments(outs[0], ins[9], ins[10])
    worst = max(float(np.max(np.abs(mean) / tol_mean)), float(np.max(np.abs(second - m2) / tol_m2)))
    key = ("post_attn", f"{form} LayerNorm moments")
    RATIOS[key] = (max(RATIOS.get(key, (0.0, 0.0))[0], worst), R.SAFETY_F32)
    assert worst <= R.SAFETY_F32, f"{what}: LayerNorm moments ratio {worst:.3f}"
    return outs


@pytest.mark.parametrize("hidden,inter", [(384, 1536), (256, 1024), (128, 512), (384, 1280)])
def test_post_attention_block(hidden, inter):
    """launch_bert_post_attn_w and its _fixed twin: the same kernel below 8,193 rows, so the same bits."""
    for m in (1, 31, 32, 33, 100):
        a = run_post_attn(0, hidden, inter, m)
        b = run_post_attn(1, hidden, inter, m)
        for u, v in zip(a, b):
            assert np.array_equal(u.view(np.uint32), v.view(np.uint32)), (hidden, inter, m)


@pytest.mark.parametrize("hidden,inter", [(384, 1536), (128, 512)])
def test_post_attention_block_across_the_64_row_switch(hidden, inter):
    """8,192 rows: the last launch of 32-row blocks; 8,193: the first of bert_ffn_w64_kernel; 8,250 leaves a 58-row tail."""
    for m in (8192, 8193, 8250):
        run_post_attn(0, hidden, inter, m)


@pytest.mark.parametrize("hidden,inter", [(256, 512), (256, 768), (384, 768), (384, 1024), (128, 256)])
def test_post_attention_as_two_launches(hidden, inter):
    """launch_bert_gemm_ln_w then launch_bert_ffn_w (bert_ffn_w_kernel<CT, 2 | 3, false>): what a model takes whose intermediate tile is
    too small to lend its LDS to the output projection; 768 / 128 = 6 tiles per wave run as chunks of three."""
    for m in (1, 31, 32, 33, 100):
        run_post_attn(2, hidden, inter, m)
    ins, _ = post_attn_case(hidden, inter)
    tiled = [ins[0][:2]] + list(ins[1:11]) + [ins[11][:2]]
    assert R.run_stage(R.POST_ATTN, 0, tiled, [(2, hidden)] * 2, m=2, hidden=hidden, inter=inter, eps=R.LN_EPS, expect=2) == 2


# ---- embedding + LayerNorm, pooling ---------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hidden", [128, 256, 384, 512, 1024])
@pytest.mark.parametrize("form", [0, 1])
def test_embedding_layer_norm(form, hidden):
    for tokens in (1, 3, 4, 5, 15, 16, 17, 33):
        ids, positions, types, word, pos, type_emb, g, beta = R.embed_inputs(tokens, hidden, 7 * hidden + tokens)
        if form == 0:
            types = np.zeros_like(types)
        refs = R.embed_ln(ids, positions, types, word, pos, type_emb, g, beta)
        outs = R.run_stage(R.EMBED_LN, form, [word, pos, type_emb, g, beta], [(tokens, hidden)] * 2, ids=ids, positions=positions, types=types,
                           m=tokens, hidden=hidden, vocab=word.shape[0], max_pos=pos.shape[0], eps=R.LN_EPS)
        check_two_copies("embed_ln", form, outs, refs, tokens, f"hidden {hidden} tokens {tokens}")
    bad = ids.copy()
    bad[0] = word.shape[0]
    assert R.run_stage(R.EMBED_LN, form, [word, pos, type_emb, g, beta], [(tokens, hidden)] * 2, ids=bad, positions=positions, types=types,
                       m=tokens, hidden=hidden, vocab=word.shape[0], max_pos=pos.shape[0], eps=R.LN_EPS, expect=2) == 2


@pytest.mark.parametrize("hidden", [128, 384, 1024])
def test_pooling(hidden):
    x, offsets = R.pool_inputs(hidden, hidden)
    ref, bound = R.pool(x, offsets)
    out, = R.run_stage(R.POOL, 0, [x], [(len(offsets) - 1, hidden)], offsets=offsets, m=x.shape[0], hidden=hidden, n_docs=len(offsets) - 1)
    check("pool", 0, out, ref, bound, f"hidden {hidden}", f16=False)
    assert np.all(out[[0, 6, 7]] == 0)   # the empty documents and the one whose mean is below the zero guard
    assert np.allclose(np.linalg.norm(out[1:6], axis=1), 1.0, atol=1e-5)

"""The two short-text forwards stage by stage, through fsgpu_lab_bert_short_stage (the embedder's own launchers, argument blocks and
row-block packing on host arrays), against the f64 references and derived bounds of tests/encoder_short_ref.py: the four launches of a
query-path layer and its pooling (bert_query_kernels.hip) at the token counts where a 16-row matrix-core tile or a 4-row LayerNorm
group ends, and the one-launch forward (bert_docs_w.hip) at one and two layers on the packings where a block fills, a text does not fit,
or a block holds more texts than it keeps boundaries for.  Pass condition: max |got - ref| / bound <= SAFETY[stage] (1 everywhere).
Then the properties the code makes exact: what shares a block or a call does not change a text's bits, workspaces keep nothing of the
call before, a replayed graph computes what an eager call computes, a repeated call repeats its bits."""
import functools
import os

import numpy as np
import pytest

import encoder_stage_ref as R
import encoder_short_ref as S

pytestmark = pytest.mark.gpu
RATIOS = {}   # (stage, output) -> largest ratio seen in this run


@pytest.fixture(scope="module", autouse=True)
def built():
    from frankensearch_amd.build import build
    build()
    yield
    path = os.environ.get("FSGPU_SHORT_RATIOS")   # (how profiles/encoder_short/ratios.txt is made)
    if path:
        with open(path, "a") as f:
            for (stage, output), (ratio, safety) in sorted(RATIOS.items()):
                f.write(f"{stage:16s} {output:12s} max ratio {ratio:.4f}  factor {safety:g}\n")


def check(stage, output, got, ref, bound, what, key):
    ratio = S.compare(got, ref, bound)
    safety = S.SAFETY[key]
    RATIOS[(stage, output)] = (max(RATIOS.get((stage, output), (0.0, 0.0))[0], ratio), safety)
    print(f"{stage} {output} {what}: ratio {ratio:.4f}")
    assert ratio <= safety, f"{stage} {output} {what}: ratio {ratio:.3f}"


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@functools.lru_cache(maxsize=None)
def layer0(family):
    """Layer 0's tensors with the matrices as the device holds them (f16-representable): what both the lab and the references get."""
    return S.as_kernel_holds(S.layer_tensors(S.weights(family), 0))


# ---- the query path's stages ------------------------------------------------------------------------------------------------------------

def run_q_attn(family, lens, form, ids=None):
    """(ctx, x_out, reference ctx, its bound) of one Q_ATTN call."""
    w = S.weights(family)
    t = layer0(family)
    offsets = S.offsets_of(lens)
    m = int(offsets[-1])
    if form == 0:
        ids = S.token_ids(m, 100 + m) if ids is None else ids
        positions = S.positions_of(offsets)
        emb = S.embedding_tensors(w)
        x, dx = S.embedding_ln(ids, positions, *emb)
        ins = emb + [t[0], t[1]]
        ctx, x_out = S.run_short_stage(S.Q_ATTN, 0, ins, [(m, S.H), (m, S.H)], offsets, ids=ids, positions=positions, vocab=S.VOCAB, max_pos=S.MAX_POS)
    else:
        x_in, parts, prev_bias = S.pending_inputs(m, 4, 200 + m)
        x, dx = S.pending_ln(x_in, parts, prev_bias, t[10], t[11])
        ctx, x_out = S.run_short_stage(S.Q_ATTN, 1, [x_in, parts, prev_bias, t[10], t[11], t[0], t[1]], [(m, S.H), (m, S.H)], offsets)
    what = f"{family} form {form} lens {list(lens)[:8]}"
    check(f"Q_ATTN form {form}", "x_out", x_out, x, dx, what, "q_attn")       # the f32 LayerNorm reference within the f32 bound
    ref, bound = S.q_attn(x, dx, t[0], t[1], offsets)
    check(f"Q_ATTN form {form}", "ctx", ctx, ref, bound, what, "q_attn")
    return ctx, x_out


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_q_attn(family, form):
    for lens in S.query_layouts():
        run_q_attn(family, lens, form)


@pytest.mark.parametrize("family", S.FAMILIES)
def test_q_gemm_out_projection(family):
    t = layer0(family)
    for m in S.Q_TOKENS:
        a = S.activation_inputs(m, S.H, 500 + m)
        slab, = S.run_short_stage(S.Q_GEMM, 0, [a, t[2]], [(m, S.H)], [0, m])
        ref, bound = S.q_gemm_plain(a, t[2])
        check("Q_GEMM form 0", "slab", slab, ref[0], bound[0], f"{family} m {m}", "q_gemm")


@pytest.mark.parametrize("family", S.FAMILIES)
def test_q_gemm_ffn_up(family):
    t = layer0(family)
    for m in S.Q_TOKENS:
        x_in, parts, prev_bias = S.pending_inputs(m, 1, 300 + m)
        tile, x_out = S.run_short_stage(S.Q_GEMM, 1, [x_in, parts, prev_bias, t[4], t[5], t[6], t[7]], [(m, S.INTER), (m, S.H)], [0, m])
        x, dx = S.pending_ln(x_in, parts, prev_bias, t[4], t[5])
        check("Q_GEMM form 1", "x_out", x_out, x, dx, f"{family} m {m}", "q_gemm")
        ref, bound = S.q_gemm_ln_gelu(x, dx, t[6], t[7])
        check("Q_GEMM form 1", "gelu tile", tile, ref, bound, f"{family} m {m}", "q_gemm")


@pytest.mark.parametrize("family", S.FAMILIES)
def test_q_gemm_ffn_down_and_its_slab_sum(family):
    t = layer0(family)
    for m in S.Q_TOKENS:
        a = S.activation_inputs(m, S.INTER, 400 + m)
        slabs, = S.run_short_stage(S.Q_GEMM, 2, [a, t[8]], [(4, m, S.H)], [0, m])
        ref, bound = S.q_gemm_plain(a, t[8])
        check("Q_GEMM form 2", "slabs", slabs, ref, bound, f"{family} m {m}", "q_gemm")
        # the four slabs, summed in f64, are the unsplit product within the f32 dot-product bound
        whole, wbound = R._dot(a, t[8], 0.0)
        check("Q_GEMM form 2", "slab sum", slabs.astype(np.float64).sum(axis=0), whole, wbound, f"{family} m {m}", "q_gemm")


@pytest.mark.parametrize("side", ["above the guard", "below the guard"])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_q_pool(family, side):
    """LayerNorm gains of the family (squared norms of ~ 10: far above POOL_GUARD), and gains of 2e-6 with no offset (squared norms
    below 1e-8, under a quarter of POOL_GUARD: exact zeros); S.pool_rows refuses an input within 4x of the guard.  Empty texts: zeros."""
    t = layer0(family)
    g, beta = (t[10], t[11]) if side == "above the guard" else (np.full(S.H, 2e-6, np.float32) * np.sign(t[10]), np.zeros(S.H, np.float32))
    for lens in S.query_layouts():
        offsets = S.offsets_of(lens)
        m = int(offsets[-1])
        x_in, parts, prev_bias = S.pending_inputs(m, 4, 200 + m)
        pooled, = S.run_short_stage(S.Q_POOL, 0, [x_in, parts, prev_bias, g, beta], [(len(lens), S.H)], offsets)
        x, dx = S.pending_ln(x_in, parts, prev_bias, g, beta)
        ref, bound = S.pool_rows(x, dx, np.zeros_like(x), offsets)
        empty = np.array(lens) == 0
        assert np.all(pooled[empty] == 0), (family, lens)
        if side == "below the guard":
            # (zeros of either sign: the kernel multiplies the mean by a scale of 0, as launch_bert_pool does)
            assert np.all(ref == 0) and np.all(pooled == 0), (family, lens)
        else:
            assert np.all(np.abs(ref[~empty]).sum(axis=1) > 0)
        check("Q_POOL", side[:5], pooled, ref, bound, f"{family} lens {list(lens)[:8]}", "q_pool")


def test_query_stages_refuse_what_the_product_never_sends():
    a, w = np.zeros((4, S.H), np.float32), np.zeros((S.H, S.H), np.float32)
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(4, S.H)], [0, 3, 5], m=4, expect=2) == 2      # offsets past m
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(4, S.H)], [0, 3, 2, 4], expect=2) == 2        # decreasing offsets
    assert S.run_short_stage(S.Q_GEMM, 0, [a, w], [(4, S.H)], [0, 4], hidden=128, inter=512, heads=4, expect=2) == 2


# ---- the one-launch forward ----------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def docs_reference(family, lens, layers):
    """(ids, offsets, pooled reference, bound): computed once per case, shared by the tests that need it, left unchanged."""
    w = S.weights(family)
    offsets = S.offsets_of(lens)
    ids = S.token_ids(int(offsets[-1]), 500 + len(lens))
    ref, bound, _ = S.docs_forward(ids, offsets, S.embedding_tensors(w), [S.as_kernel_holds(S.layer_tensors(w, l)) for l in range(layers)])
    for a in (ids, offsets, ref, bound):
        a.setflags(write=False)
    return ids, offsets, ref, bound


@pytest.mark.parametrize("layers", [1, 2])
@pytest.mark.parametrize("family", S.FAMILIES)
def test_docs_layers(family, layers):
    for lens in S.DOCS_LAYOUTS:
        assert sum(lens) > 32 and max(lens) <= 32     # the product's predicate for this path
        ids, offsets, ref, bound = docs_reference(family, tuple(lens), layers)
        pooled = S.run_docs(ids, offsets, S.weights(family), layers)
        assert np.all(pooled[np.array(lens) == 0] == 0), (family, lens)
        check(f"DOCS {layers} layer{'s' * (layers > 1)}", "pooled", pooled, ref, bound, f"{family} lens {list(lens)[:6]}.. ({len(lens)} texts)", "docs")


def texts_of(ids, offsets):
    return [np.asarray(ids[a:b]).tolist() for a, b in zip(offsets[:-1], offsets[1:])]


@pytest.fixture(scope="module")
def six_layers():
    """(weights, embedder) of the MiniLM-L6 shape: the embedder the exact properties run on."""
    import frankensearch_amd as fa
    w = S.weights("random", 6, 9)
    m = fa.NativeEmbedder(w)
    yield w, m
    m.close()


def test_docs_six_layers_lab_route_equals_the_embedder(six_layers):
    """All six layers once: the lab route and NativeEmbedder agree bit for bit on the same weights and texts (the packing, the argument
    block and the weight preparation are the product's), and both hold the end-to-end tolerance of tests/test_gpu_bert.py."""
    from oracle import bert_oracle
    w, m = six_layers
    lens = [0, 0, 5, 0, 27, 6, 0, 0, 31, 2, 0]
    offsets = S.offsets_of(lens)
    ids = S.token_ids(int(offsets[-1]), 77)
    lab = S.run_docs(ids, offsets, w, 6)
    got = m.embed_batch_token_ids(texts_of(ids, offsets))
    assert np.array_equal(bits(lab), bits(got))
    want = bert_oracle.CForward(w, 6).run(texts_of(ids, offsets), 8)
    assert np.max(np.abs(lab - want)) <= 2e-3
    nz = np.array(lens) > 0
    assert np.all(np.sum(lab[nz] * want[nz], axis=1) >= 0.999) and np.all(lab[~nz] == 0)


# ---- exact properties -----------------------------------------------------------------------------------------------------------------------

def other_ids(ids, offsets, keep, seed):
    """The same texts with the token ids of every text but `keep` replaced (lengths and places kept)."""
    out = S.token_ids(len(ids), seed).copy()
    assert np.any(out != ids)
    for d in keep:
        out[offsets[d]:offsets[d + 1]] = ids[offsets[d]:offsets[d + 1]]
    return out


def rows_of(offsets, texts):
    return np.concatenate([np.arange(offsets[d], offsets[d + 1]) for d in texts])


@pytest.mark.parametrize("family", S.FAMILIES)
def test_neighbour_independence_q_attn(family):
    """Masked probabilities are exact zeros and the rows of a linear are independent: the context rows of a text keep their bits when
    the ids of every other text of the call change."""
    for lens, keep in (([15, 17], [0]), ([17, 15], [1]), ([0, 5, 0, 27, 0], [1]), ([1] * 32, [0, 15, 16, 31]), ([31, 1], [1])):
        offsets = S.offsets_of(lens)
        m = int(offsets[-1])
        ids = S.token_ids(m, 100 + m)
        ctx, x_out = run_q_attn(family, lens, 0, ids)
        ctx2, x_out2 = run_q_attn(family, lens, 0, other_ids(ids, offsets, keep, 900 + m))
        rows = rows_of(offsets, keep)
        assert np.array_equal(bits(ctx[rows]), bits(ctx2[rows])) and np.array_equal(bits(x_out[rows]), bits(x_out2[rows])), (family, lens)
        assert not np.array_equal(bits(ctx), bits(ctx2))


@pytest.mark.parametrize("family", S.FAMILIES)
def test_neighbour_independence_docs(family):
    w = S.weights(family)
    for lens, keep in (([16, 16, 15, 17, 17, 15], [1, 3, 4]), ([1] * 33, [0, 16, 31, 32]), ([32, 2] + [0] * 93 + [10, 10, 10], [95, 97]),
                       ([0, 0, 5, 0, 27, 6, 0, 0, 31, 2, 0], [4, 9])):
        offsets = S.offsets_of(lens)
        ids = S.token_ids(int(offsets[-1]), 500 + len(lens))
        a = S.run_docs(ids, offsets, w, 2)
        b = S.run_docs(other_ids(ids, offsets, keep, 901), offsets, w, 2)
        assert np.array_equal(bits(a[keep]), bits(b[keep])), (family, lens)
        assert not np.array_equal(bits(a), bits(b))
        again = S.run_docs(ids, offsets, w, 2)           # repeats: the same call twice gives equal bits
        assert np.array_equal(bits(a), bits(again)), (family, lens)


def test_neighbour_independence_embedder_both_paths(six_layers):
    _, m = six_layers
    for lens, keep in (([5, 0, 4, 12, 11], [2, 4]), ([0, 3, 0, 1, 28], [1, 3]),                       # query path (<= 32 tokens)
                       ([16, 16, 15, 17, 17, 15], [1, 3, 4]), ([32] + [3] + [0] * 200 + [29], [1, 202])):  # one-launch path
        offsets = S.offsets_of(lens)
        ids = S.token_ids(int(offsets[-1]), 600 + len(lens))
        a = m.embed_batch_token_ids(texts_of(ids, offsets))
        b = m.embed_batch_token_ids(texts_of(other_ids(ids, offsets, keep, 902), offsets))
        assert np.array_equal(bits(a[keep]), bits(b[keep])), lens
        assert not np.array_equal(bits(a), bits(b))


def fresh(w, texts):
    import frankensearch_amd as fa
    m = fa.NativeEmbedder(w)
    out = m.embed_batch_token_ids(texts)
    m.close()
    return out


def test_stale_workspaces(six_layers):
    """Workspaces keep the rows of the previous, longer call: a 3-token query after a 32-token one, [5, 0, 4] after [10, 10, 12] —
    bit-equal to the same calls on a fresh embedder."""
    import frankensearch_amd as fa
    w, _ = six_layers
    m = fa.NativeEmbedder(w)
    calls = [[32], [3], [10, 10, 12], [5, 0, 4]]
    for i, lens in enumerate(calls):
        offsets = S.offsets_of(lens)
        texts = texts_of(S.token_ids(int(offsets[-1]), 700 + i), offsets)
        got = m.embed_batch_token_ids(texts)
        assert np.array_equal(bits(got), bits(fresh(w, texts))), lens
    m.close()


def test_graph_replay_of_other_splits_of_the_same_shape(six_layers):
    """The graph cache is keyed by (texts, tokens, longest text): n = 3, total = 20, max_seq = 10 as four different splits and ids on one
    embedder — an eager run, the capture, two replays — each bit-equal to a fresh embedder's eager call of the same input."""
    import frankensearch_amd as fa
    w, _ = six_layers
    m = fa.NativeEmbedder(w)
    for i, lens in enumerate(([10, 5, 5], [5, 10, 5], [5, 5, 10], [10, 5, 5])):
        offsets = S.offsets_of(lens)
        texts = texts_of(S.token_ids(20, 800 + i), offsets)
        got = m.embed_batch_token_ids(texts)
        assert np.array_equal(bits(got), bits(fresh(w, texts))), (i, lens)
    m.close()

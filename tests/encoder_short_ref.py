"""Plain numpy f64 references of the two short-text forwards' stages (bert_query_kernels.hip: Q_ATTN, Q_GEMM, Q_POOL; bert_docs_w.hip:
DOCS, the whole forward of `layers` layers), their per-element error bounds, and the inputs of tests/test_gpu_encoder_short.py.

Built on tests/encoder_stage_ref.py (same unit roundoffs U16 / U32 / SUB16, same comparator).  A reference rounds where the kernel is
documented to round — the f16 A tile behind a LayerNorm prologue, f16 Q, K and V, the f16 probabilities, the f16 context and GELU tile,
f32 everywhere else — and its bound is computed from its own f64 intermediates only, never from a GPU output.  Where a stage chains
roundings, a value's uncertainty is carried through the next step as encoder_stage_ref.post_attn does: an f16 tile element that lies
within its own error of a rounding boundary may round the other way in the kernel (_store16), and the disagreements of a tile row are
carried through a projection at TILE_CONF standard deviations; every other term is a worst-case sum.

Pass condition: compare(got, ref, bound) <= SAFETY[stage] — 1 for every output here (f32 outputs and compositions of several roundings;
profiles/encoder_short/ratios.txt has the measured maxima).  The module imports without a GPU: tests/test_encoder_short_contract.py
checks the references against oracle.bert_oracle and, with faulty references in place of the GPU, that no fault of its list passes.
"""
import functools

import numpy as np

import encoder_stage_ref as R
from encoder_stage_ref import U16, U32, SUB16, TILE_CONF, ATTN_SCALE, LN_EPS, POOL_GUARD, compare, h16, offsets_of  # noqa: F401

H, INTER, HEADS = 384, 1536, 12
Q_ATTN, Q_GEMM, Q_POOL, DOCS = range(4)
SAFETY = {"q_attn": 1.0, "q_gemm": 1.0, "q_pool": 1.0, "docs": 1.0}
LAYER_KEYS = ["attention.output.dense.weight", "attention.output.dense.bias", "attention.output.LayerNorm.weight",
              "attention.output.LayerNorm.bias", "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight",
              "output.dense.bias", "output.LayerNorm.weight", "output.LayerNorm.bias"]


# ---- pieces -------------------------------------------------------------------------------------------------------------------------
# An intermediate value is carried as (v, det, var): the kernel's value differs from the reference's v by at most det + a zero-mean
# term of variance var.  det collects what is summed at its worst (f32 arithmetic, the stores themselves); var collects the
# disagreements of f16 tiles, which are whole ulps of either sign, independent from element to element (encoder_stage_ref.post_attn:
# "which way an element rounds depends on where its own value lies between its own two neighbours").  total() is the bound.

def total(det, var):
    return det + TILE_CONF * np.sqrt(var)


def store16(v, det, var):
    """v stored as f16.  The kernel's stored value is the reference's r16(v) unless a rounding boundary lies between the two
    unrounded values; then it is whole ulps away — one, unless the error itself is larger than an ulp.  With `dist` the distance from
    v to its nearest boundary, a disagreement takes an error above dist: excluded when det + TILE_CONF sqrt(var) < dist.  Otherwise
    the error is taken as a zero-mean normal term: det is a sum of many independent f32 roundings all given the same sign, so it counts
    as TILE_CONF standard deviations (variance var + (det / TILE_CONF)^2), and a boundary is crossed with the probability that the
    term exceeds dist towards the nearest boundary or ulp - dist towards the other one (the 7.1.26 erf is good to 1.5e-7, added).
    The stored disagreement's variance is at most that variance + ulp^2 x the probability (small errors: an ulp with that
    probability; errors beyond an ulp: their own variance plus the rounding's).
    Returns (stored value, var): with var = 0 the exclusion is encoder_stage_ref._store16's test."""
    h = R.r16(v)
    ulp = np.spacing(np.abs(h).astype(np.float16)).astype(np.float64)
    pow2 = np.frexp(h)[0] == 0.5
    half = np.where(pow2 & (np.abs(v) < np.abs(h)), ulp / 4, ulp / 2)
    dist = np.maximum(half - np.abs(v - h), 0.0)
    var = var + (det / TILE_CONF) ** 2
    sd = np.sqrt(np.where(var > 0, var, 1.0) * 2.0)

    def tail(room):
        return np.where(var > 0, 0.5 * (1.0 - R._erf_as(np.maximum(room, 0.0) / sd)) + 1e-7, 0.0)

    prob = np.minimum(tail(dist) + tail(ulp - dist), 1.0)
    return h, np.where(TILE_CONF * np.sqrt(var) < dist, 0.0, var + ulp * ulp * prob)


def project(xh, var_xh, w, b):
    """An f16 tile (disagreeing by var_xh) through w [N, K] f16 and an f32 bias in f32: (y, det, var)."""
    y, dy = R._dot(xh, w, b)
    w = np.asarray(w, np.float64)
    return y, dy, var_xh @ (w * w).T


def layer_norm(y, det, var, g, beta, eps=LN_EPS):
    """LayerNorm of rows known to (det, var).  det goes through encoder_stage_ref.layer_norm's worst-case model with the f32 arithmetic;
    the independent part through the derivative d out_i / d y_k = g_i inv (1[i = k] - 1 / H - d_i d_k / (H (V + eps))), d = y - mean,
    V the variance: var_out_i = sum_k of its square times var_k.  Returns (out, det, var)."""
    out, bound = R.layer_norm(y, det, g, beta, eps)
    y, g = np.asarray(y, np.float64), np.asarray(g, np.float64)
    n = y.shape[-1]
    d = y - y.mean(axis=-1, keepdims=True)
    v = (d * d).mean(axis=-1, keepdims=True) + eps
    inv2 = 1.0 / v
    c = d / (n * v)                                             # d out_i / d y_k = g_i inv (1[i = k] - 1 / n - d_i c_k)
    s0 = var.sum(axis=-1, keepdims=True) / (n * n)
    s1 = (c * var).sum(axis=-1, keepdims=True) / n
    s2 = (c * c * var).sum(axis=-1, keepdims=True)
    own = var * (1.0 - 2.0 / n - 2.0 * d * c)
    var_out = g * g * inv2 * np.maximum(own + s0 + 2 * d * s1 + d * d * s2, 0.0)
    return out, bound, var_out


def pending_ln(x_in, parts, prev_bias, g, beta, eps=LN_EPS):
    """The prologue of a consumer stage (q_ln_rows): LayerNorm(x_in + (prev_bias + slab 0 + slab 1 ...)), the slabs added to the bias in
    order and the residual last: len(parts) + 1 f32 additions, each to U32 of its own result, all of them at most
    |x_in| + |prev_bias| + sum |slab|; then encoder_stage_ref.layer_norm's model (two passes, a row sum 12 additions deep: six in a lane,
    two inside a float4, four across the 16 lanes).  parts [slabs, m, H].  Returns (x, bound): the f32 rows the stage stores as x_out."""
    x_in, parts, prev_bias = (np.asarray(a, np.float64) for a in (x_in, parts, prev_bias))
    v = x_in + prev_bias + parts.sum(axis=0)
    dv = (parts.shape[0] + 1) * U32 * (np.abs(x_in) + np.abs(prev_bias) + np.abs(parts).sum(axis=0))
    return R.layer_norm(v, dv, g, beta, eps)


def embedding_ln(ids, positions, word, pos, type0, g, beta, eps=LN_EPS):
    """LayerNorm((word[id] + pos[p]) + type0): the embedding prologue of both forwards.  Returns (x, bound)."""
    out, bound, _ = R.embed_ln(ids, positions, np.zeros(len(ids), np.int64), word, pos, np.asarray(type0).reshape(1, -1), g, beta, eps)
    return out, bound


def attention_texts(q, var_q, k, var_k, v, var_v, offsets, scale=ATTN_SCALE):
    """softmax(scale q k^T) v per text and head over f16 Q, K, V [m, H] that disagree with the kernel's by var_q, var_k, var_v.
    encoder_stage_ref.attend (with p_f16 = False) bounds the f32 arithmetic on exact operands (scores, exponentials, the P V product)
    and the f16 store: the det part.  The probabilities are rounded to f16 one by one before P V — unnormalised in the one-launch
    kernel, whose largest is 1, normalised in the query kernel: U16 relative and SUB16 absolute against a row sum >= 1 either way —,
    each rounding of either sign and at most U16 p_ij: var U16^2 sum_j p_ij^2 v_jd^2 + SUB16^2 sum_j v_jd^2 (summed at their worst
    they alone would exceed the half ulp of the context they are stored into).  The operands' disagreements go through the derivative of a softmax-weighted mean,
    d o_id = sum_j p_ij (scale (v_jd - o_id) d s_ij + d v_jd) with d s_ij = sum_e (d q_ie k_je + q_ie d k_je):
      var_o_id = scale^2 (sum_e var_q_ie (sum_j p_ij (v_jd - o_id) k_je)^2 + sum_j p_ij^2 (v_jd - o_id)^2 sum_e q_ie^2 var_k_je) + sum_j p_ij^2 var_v_jd
    Returns (ctx [m, H], det with the f16 store, det before the store, var)."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    ctx, det, var = np.zeros_like(q), np.zeros_like(q), np.zeros_like(q)
    for d in range(len(offsets) - 1):
        a, b = int(offsets[d]), int(offsets[d + 1])
        if a == b:
            continue
        for h in range(HEADS):
            c = slice(32 * h, 32 * h + 32)
            qq, kk, vv = q[a:b, c], k[a:b, c], v[a:b, c]
            o, bd = R.attend(qq, kk, vv, scale, p_f16=False)
            s = qq @ kk.T
            p = np.exp((s - s.max(axis=1, keepdims=True)) * scale)
            p /= p.sum(axis=1, keepdims=True)
            spread = vv[None, :, :] - o[:, None, :]                                # [query i, key j, dim d]
            lever = np.einsum("ij,ijd,je->ide", p, spread, kk)                      # sum_j p_ij (v_jd - o_id) k_je
            from_q = np.einsum("ie,ide->id", var_q[a:b, c], lever * lever)
            from_k = np.einsum("ij,ijd,ij->id", p * p, spread * spread, (qq * qq) @ var_k[a:b, c].T)
            ctx[a:b, c], det[a:b, c] = o, bd
            p_tile = U16 * U16 * ((p * p) @ (vv * vv)) + SUB16 * SUB16 * (vv * vv).sum(axis=0, keepdims=True)
            var[a:b, c] = scale * scale * (from_q + from_k) + (p * p) @ var_v[a:b, c] + p_tile
    return ctx, det, np.maximum(det - U16 * np.abs(ctx) - SUB16, 0.0), var


def _gelu_grad(x):
    return np.abs(0.5 * (1.0 + R._erf_as(x * 0.70710678118654752440)) + x * np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)) + 1e-6


def q_gelu_bound(x, dx):
    """q_gelu (bert_query_kernels.hip) is the Abramowitz-Stegun 7.1.26 form itself, in f32 with __expf, against the same form in f64
    (encoder_stage_ref.gelu).  From the formula: z and t = 1 / (1 + 0.3275911 |z|) to 1 and 3 U32 relative; the Horner polynomial
    (coefficients of magnitude up to 1.45, t <= 1, alternating signs) to 10 U32 absolute on a value <= 1; __expf(-z^2) = exp2(-z^2 log2 e)
    to (2 z^2 + 4) U32 relative, i.e. at most 5 U32 absolute (z^2 exp(-z^2) <= 0.37); 1 - poly exp and 1 + erf one U32 each: 20 U32 on
    1 + erf, times |x| / 2; the last two multiplications 4 U32 relative; and |gelu'| dx (|gelu'| <= 1.13) for an argument known to dx.
    No fitted polynomial here: encoder_stage_ref.ERF_FIT belongs to the packed kernels' GELU and is not part of this bound."""
    return _gelu_grad(x) * dx + 0.5 * np.abs(x) * 20 * U32 + 4 * U32 * np.abs(R.gelu(x))


def docs_gelu_f64(x):
    """d_gelu of bert_docs_w.hip (the coefficients of gelu_as_w, bert_gemm_w.hip) in f64: what ERF_FIT is measured on."""
    x = np.asarray(x, np.float64)
    az = np.abs(x) * 0.70710678118654752440
    p = az * -0.00294418 + 0.02959011
    for c in (-0.14866571, -0.91850934, -1.62788901):
        p = p * az + c
    return np.maximum(x, 0.0) - np.abs(x) * np.exp2(p * az - 1.0)


def pool_rows(x, det, var, offsets):
    """Mean over a text's rows, then L2 with the zero guard, for rows known to (det, var) (q_pool_compute and the tail of
    bert_docs_w_kernel: thread d adds the text's n <= 32 rows in order and multiplies by 1 / n: (n + 2) U32 mean |x|; the squared norm
    over 384 dimensions in a tree at most 12 deep, 2 sum |val| dval + 24 U32 norm_sq; its inverse root half of that + 4 U32 relative;
    the independent part through d out = s (d val - out (out . d val))).  A text whose squared norm is at or below POOL_GUARD, or an
    empty text, gives exact zeros (bound 0).  Returns (out [n_docs, H], bound)."""
    x, det, var = (np.asarray(a, np.float64) for a in (x, det, var))
    n_docs = len(offsets) - 1
    out = np.zeros((n_docs, x.shape[1]))
    bound = np.zeros_like(out)
    for d in range(n_docs):
        a, b = int(offsets[d]), int(offsets[d + 1])
        if a == b:
            continue
        n = b - a
        val = x[a:b].sum(axis=0) / n
        dval = (n + 2) * U32 * np.abs(x[a:b]).sum(axis=0) / n + det[a:b].sum(axis=0) / n
        vval = var[a:b].sum(axis=0) / (n * n)
        nsq = float((val * val).sum())
        dnsq = 2 * float((np.abs(val) * total(dval, vval)).sum()) + 24 * U32 * nsq
        assert nsq >= 4 * POOL_GUARD + 4 * dnsq or nsq <= POOL_GUARD / 4 - 4 * dnsq, "test input sits near the zero guard"
        if nsq <= POOL_GUARD:
            continue
        s = 1.0 / np.sqrt(nsq)
        out[d] = val * s
        dnsq = 2 * float((np.abs(val) * dval).sum()) + 24 * U32 * nsq
        vout = s * s * (vval * (1 - 2 * out[d] ** 2) + out[d] ** 2 * float((out[d] ** 2 * vval).sum()))
        bound[d] = total(dval * s + np.abs(out[d]) * (dnsq / (2 * nsq) + 4 * U32), np.maximum(vout, 0.0))
    return out, bound


# ---- the six query stages -----------------------------------------------------------------------------------------------------------

def qkv16(x, det, var, wqkv, bqkv):
    """The f16 x tile of rows known to (det, var) through the stacked [1152, 384] projection, Q, K and V stored as f16:
    three (stored value, var)."""
    xh, var_xh = store16(x, det, var)
    wqkv, bqkv = np.asarray(wqkv, np.float64), np.asarray(bqkv, np.float64)
    out = []
    for part in range(3):
        out += store16(*project(xh, var_xh, wqkv[part * H:(part + 1) * H], bqkv[part * H:(part + 1) * H]))
    return out


def q_attn(x, dx, wqkv, bqkv, offsets, scale=ATTN_SCALE):
    """K1 behind its prologue: x [m, H] are the prologue's f32 rows (pending_ln or embedding_ln), known to dx.  f16 A tile, the head's
    Q, K, V columns f16, attention per text.  Returns (ctx, bound)."""
    ctx, det, _, var = attention_texts(*qkv16(x, dx, np.zeros_like(x), wqkv, bqkv), offsets, scale)
    return ctx, total(det, var)


def q_gemm_plain(a, w):
    """Modes 0 and 2: a [m, K] f16 x w [N, K]^T in slabs of 384 along K, f32, no bias.  Returns (slabs [K / 384, m, N], bounds)."""
    a, w = np.asarray(a, np.float64), np.asarray(w, np.float64)
    out = [R._dot(a[:, k0:k0 + H], w[:, k0:k0 + H], 0.0) for k0 in range(0, a.shape[1], H)]
    return np.stack([o[0] for o in out]), np.stack([o[1] for o in out])


def q_gemm_ln_gelu(x, dx, w, bias):
    """Mode 1 behind its prologue: f16 A tile of the LayerNorm rows x (known to dx), w [1536, 384], + bias, q_gelu, stored f16.
    Returns (gelu tile, bound)."""
    xh, var_xh = store16(x, dx, np.zeros_like(x))
    u, du, vu = project(xh, var_xh, w, bias)
    g = R.gelu(u)
    return g, total(q_gelu_bound(u, du) + U16 * np.abs(g) + SUB16, _gelu_grad(u) ** 2 * vu)


# ---- the one-launch forward ----------------------------------------------------------------------------------------------------------

def layer_tensors(weights, layer):
    """The twelve tensors of a layer in the lab's order (stacked Q | K | V first), f32, from HuggingFace-layout weights."""
    w = {(k[5:] if k.startswith("bert.") else k): v for k, v in weights.items()}
    p = f"encoder.layer.{layer}."
    qkv_w = np.concatenate([w[p + f"attention.self.{n}.weight"] for n in ("query", "key", "value")], axis=0)
    qkv_b = np.concatenate([w[p + f"attention.self.{n}.bias"] for n in ("query", "key", "value")], axis=0)
    return [np.ascontiguousarray(t, np.float32) for t in [qkv_w, qkv_b] + [w[p + k] for k in LAYER_KEYS]]


def embedding_tensors(weights):
    w = {(k[5:] if k.startswith("bert.") else k): v for k, v in weights.items()}
    return [np.ascontiguousarray(t, np.float32) for t in (
        w["embeddings.word_embeddings.weight"], w["embeddings.position_embeddings.weight"], w["embeddings.token_type_embeddings.weight"][0],
        w["embeddings.LayerNorm.weight"], w["embeddings.LayerNorm.bias"])]


def positions_of(offsets):
    """Positions restart at 0 at every text's start."""
    return np.concatenate([np.arange(int(b) - int(a)) for a, b in zip(offsets[:-1], offsets[1:])] + [np.zeros(0, int)]).astype(np.int32)


def docs_layer(x, det, var, t, offsets, eps=LN_EPS, scale=ATTN_SCALE):
    """One encoder layer of the one-launch kernel on rows x known to (det, var); t = layer_tensors (matrices as the kernel holds them:
    f16).  QKV from the f16 x tile, f16 Q, K, V, attention, f16 context; x1 = LayerNorm(x + ctx Wao^T + b) f32 with its f16 copy as the
    x tile; GELU (the fitted form: encoder_stage_ref._gelu_bound with packed = True) tile f16; x = LayerNorm(x1 + g W2^T + b2).  The
    residual's own uncertainty rides along with the projection's (taken as independent of it).
    Returns (x, det, var, y) — y the rows the last LayerNorm normalised (for encoder_stage_ref._moment_tolerances)."""
    wqkv, bqkv, wao, bao, ln1w, ln1b, w1, b1, w2, b2, ln2w, ln2b = (np.asarray(a, np.float64) for a in t)
    ctx, _, dctx, vctx = attention_texts(*qkv16(x, det, var, wqkv, bqkv), offsets, scale)
    ch, vch = store16(ctx, dctx, vctx)
    lin, dl, vl = project(ch, vch, wao, bao)
    y1 = lin + x
    x1, d1, v1 = layer_norm(y1, dl + det + 2 * U32 * (np.abs(lin) + np.abs(y1)), vl + var, ln1w, ln1b, eps)
    x1h, vx1h = store16(x1, d1, v1)
    u, du, vu = project(x1h, vx1h, w1, b1)
    gh, vgh = store16(R.gelu(u), R._gelu_bound(u, du, True), _gelu_grad(u) ** 2 * vu)
    lin2, dl2, vl2 = project(gh, vgh, w2, b2)
    y2 = lin2 + x1
    out, dout, vout = layer_norm(y2, dl2 + d1 + 2 * U32 * (np.abs(lin2) + np.abs(y2)), vl2 + v1, ln2w, ln2b, eps)
    return out, dout, vout, y2


def docs_forward(ids, offsets, emb, layers, eps=LN_EPS, scale=ATTN_SCALE, positions=None, attn_offsets=None, pool_offsets=None):
    """The whole forward of len(layers) layers: emb = embedding_tensors, layers = [layer_tensors with f16-representable matrices].
    positions / attn_offsets / pool_offsets: what a FAULTY kernel would use in place of the texts' own (the contract test).
    Returns (pooled [n_docs, H], bound, (x, bound of x, y) of the last layer)."""
    positions = positions_of(offsets) if positions is None else positions
    x, det = embedding_ln(ids, positions, *emb, eps)
    var, y = np.zeros_like(x), None
    for t in layers:
        x, det, var, y = docs_layer(x, det, var, t, offsets if attn_offsets is None else attn_offsets, eps, scale)
    pooled, bound = pool_rows(x, det, var, offsets if pool_offsets is None else pool_offsets)
    return pooled, bound, (x, total(det, var), y)


def as_kernel_holds(t):
    """layer_tensors with the four matrices rounded to f16 (what the device keeps), vectors untouched."""
    return [h16(a) if a.ndim == 2 else a for a in t]


# ---- the inputs of the GPU tests (the contract test puts faulty references on the same ones) ------------------------------------------

Q_TOKENS = [1, 2, 15, 16, 17, 31, 32]
Q_LAYOUTS = [[16, 16], [15, 17], [17, 15], [31, 1], [1, 31], [0, 5, 0, 27, 0], [3] + [0] * 17 + [1] + [0] * 20 + [7]]
DOCS_LAYOUTS = [[32, 32, 1], [1] * 33, [16, 16, 15, 17, 17, 15], [31, 1, 1, 31], [0, 0, 5, 0, 27, 6, 0, 0, 31, 2, 0],
                [32] + [0] * 94 + [10, 10, 10] + [0] * 5, [32] + [0] * 96 + [20, 12], [32] + [3] + [0] * 200 + [29],
                # empty texts stay in the block in front of them, so two more: non-empty texts at in-block indices 94, 95, 96 (the last
                # boundaries kept in LDS and the first read in place), and a block of 257 texts (an in-block index that counted empty
                # texts would no longer fit its 8 bits)
                [32, 2] + [0] * 93 + [10, 10, 10], [32, 2] + [0] * 255 + [30]]
FAMILIES = ["random", "heavy"]
VOCAB, MAX_POS = 300, 64


def query_layouts():
    """Every text layout of the query stages: one text and one-token texts at each m, then the fixed ones (40 texts, mostly empty, last)."""
    return [[m] for m in Q_TOKENS] + [[1] * m for m in Q_TOKENS if m > 1] + Q_LAYOUTS


@functools.lru_cache(maxsize=None)
def weights(family, layers=2, seed=5):
    """HuggingFace-layout weights of the MiniLM-L6 shape with a small vocabulary: oracle.bert_oracle's two families."""
    from oracle import bert_oracle as O
    make = O.random_weights if family == "random" else O.heavy_tailed_weights
    w = make(seed, VOCAB, H, layers, INTER, MAX_POS)
    for a in w.values():
        a.setflags(write=False)
    return w


def token_ids(total, seed):
    return np.random.default_rng(seed).integers(0, VOCAB, max(total, 1)).astype(np.int32)[:total]


def pending_inputs(m, slabs, seed, gain=1.0):
    """x_in [m, H], parts [slabs, m, H], prev_bias: a residual stream of ~ 1 with row i scaled by 1 + i mod 3 (a row from the other 16-row
    tile shows), slabs of ~ 0.5 each scaled differently (a slab dropped or counted twice shows), a bias of ~ 0.5."""
    rng = np.random.default_rng(seed)
    x_in = (rng.standard_normal((m, H)) * (1 + np.arange(m) % 3)[:, None]).astype(np.float32)
    parts = (rng.standard_normal((slabs, m, H)) * (0.5 + 0.25 * np.arange(slabs))[:, None, None]).astype(np.float32)
    prev_bias = (0.5 * rng.standard_normal(H)).astype(np.float32)
    return x_in, parts, prev_bias


def activation_inputs(m, k, seed):
    """a [m, k] f16-representable, row i scaled by 1 + i mod 7."""
    rng = np.random.default_rng(seed)
    return h16(rng.standard_normal((m, k)) * (1 + np.arange(m) % 7)[:, None])


# ---- the lab entry point --------------------------------------------------------------------------------------------------------------

def run_short_stage(stage, form, ins, out_shapes, offsets, ids=None, positions=None, layer_in=None, expect=0, **scalars):
    """fsgpu_lab_bert_short_stage on host arrays: ins = the f32 inputs in the header's order, layer_in = [layer_tensors, ...] (DOCS),
    out_shapes = shapes of out0 (and out1).  Returns the outputs (f32), or the status when it is not `expect`ed to be FSGPU_OK."""
    import ctypes
    from frankensearch_amd import _lib
    a = _lib.BertShortArgs()
    a.stage, a.form = stage, form
    a.hidden, a.inter, a.heads, a.eps, a.scale = H, INTER, HEADS, LN_EPS, ATTN_SCALE
    offsets = np.ascontiguousarray(offsets, np.uint32)
    a.n_docs, a.m = len(offsets) - 1, int(offsets[-1])
    a.offsets = offsets.ctypes.data
    for name, value in scalars.items():
        setattr(a, name, value)
    keep = [np.ascontiguousarray(x, np.float32) for x in ins]
    for i, x in enumerate(keep):
        a.in_[i] = x.ctypes.data
    for name, arr in (("ids", ids), ("positions", positions)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, np.int32)
            keep.append(arr)
            setattr(a, name, arr.ctypes.data)
    if layer_in is not None:
        flat = [np.ascontiguousarray(t, np.float32) for layer in layer_in for t in layer]
        table = (ctypes.c_void_p * len(flat))(*[t.ctypes.data for t in flat])
        keep += flat + [table]
        a.layers = len(layer_in)
        a.layer_in = ctypes.cast(table, ctypes.c_void_p)
    outs = [np.full(shape, np.nan, np.float32) for shape in out_shapes]
    a.out0 = outs[0].ctypes.data
    if len(outs) > 1:
        a.out1 = outs[1].ctypes.data
    status = _lib.lib().fsgpu_lab_bert_short_stage(0, ctypes.byref(a))
    if expect != 0 or status != 0:
        assert status == expect, (status, _lib.last_error())
        return status
    return outs


def run_docs(ids, offsets, w, layers, expect=0):
    """The DOCS stage on HuggingFace-layout weights w, the first `layers` layers.  Returns pooled [n_docs, H]."""
    emb = embedding_tensors(w)
    res = run_short_stage(DOCS, 0, emb, [(len(offsets) - 1, H)], offsets, ids=ids, layer_in=[layer_tensors(w, l) for l in range(layers)],
                          vocab=emb[0].shape[0], max_pos=min(emb[1].shape[0], 512), expect=expect)
    return res if isinstance(res, int) else res[0]

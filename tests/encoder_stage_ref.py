"""Plain numpy f64 references of the f16 encoder's stages, their per-element error bounds, and the inputs of the stage tests.

Every reference takes the operands the kernel sees (the test rounds to f16 on the host wherever the product holds f16) and returns the
f64 result together with a bound computed from its own f64 intermediates alone, never from a GPU output.  A bound is the sum of the
roundings the kernel is documented to perform, each at its unit roundoff:

  U16 = 2^-11  every f16 store (the softmax P tile, contexts, the GELU tile, f16 outputs) — plus SUB16 = 2^-25 absolute, the f16
               subnormal spacing, so that values below 2^-14 are covered too
  U32 = 2^-24  f32 arithmetic: K U32 sum |a_k w_k| for an f32-accumulated dot product of length K, a few U32 for every other step

`compare(got, ref, bound)` is max |got - ref| / bound; a test passes when that ratio is at most SAFETY[stage] (SAFETY_F32 for an f32
output): the factors of profiles/encoder_stages/ratios.txt, at most 4, chosen so that the largest measured ratio is at most half of them.  The module imports
without a GPU: tests/test_encoder_stage_contract.py runs the references against oracle.bert_oracle and checks, with mutated references
standing in for the GPU, that the comparator is not blind.
"""
import numpy as np

U16 = 2.0 ** -11
U32 = 2.0 ** -24
SUB16 = 2.0 ** -25
ATTN_SCALE = float(np.float32(0.17677669))   # what the product passes (1 / sqrt(32) as f32)
POOL_GUARD = float(np.float32(1.1920929e-7))  # f32::EPSILON: a squared norm at or below it pools to zeros
LN_EPS = 1e-12
ERF_FIT = 1.1e-6   # |erf fit - A&S 7.1.26| of the packed kernels' GELU (bert_gemm_w.hip, gelu_as_w: "1.1e-6 against the reference")

# Pass condition: ratio <= SAFETY[stage] for an output stored as f16, <= SAFETY_F32 for an f32 output.  Measured maxima on an MI355X:
# profiles/encoder_stages/ratios.txt.  An f16 store's bound is tight (a value just above a power of two, rounded by half an ulp, IS U16
# away), so every stage whose f16 output follows its arithmetic directly measures ~ 1.0 and gets the factor 2 that puts the
# measurement at half of it; f32 outputs, the pooling and the post-attention block measure under 0.2 and are held to the bare bound.
SAFETY = {"attention": 2.0, "linear": 2.0, "linear_ln": 2.0, "post_attn": 1.0, "embed_ln": 2.0, "pool": 1.0}
SAFETY_F32 = 1.0

ATTENTION, LINEAR, LINEAR_LN, POST_ATTN, EMBED_LN, POOL = range(6)


def r16(x):
    """Round to nearest-even f16, as f64."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float64)


def h16(x):
    """f32 array holding f16-representable values: a host input the product holds as f16."""
    return np.asarray(x, np.float64).astype(np.float16).astype(np.float32)


def compare(got, ref, bound):
    """max |got - ref| / bound.  Where the bound is 0 the value must be exact; a NaN or Inf in `got` is an infinite ratio."""
    got, ref, bound = (np.asarray(a, np.float64) for a in (got, ref, bound))
    assert got.shape == ref.shape == bound.shape, (got.shape, ref.shape, bound.shape)
    if got.size == 0:
        return 0.0
    d = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, d / bound, np.where(d == 0, 0.0, np.inf))
    ratio = np.where(np.isfinite(got), ratio, np.inf)
    return float(np.max(ratio))


def is_rne_f16_of(x_h, x_f32):
    """The exact check of every stage that returns both copies: x_h is the round-to-nearest-even f16 of the x_f32 of the same call."""
    return np.array_equal(np.asarray(x_f32, np.float32).astype(np.float16).view(np.uint16),
                          np.asarray(x_h, np.float32).astype(np.float16).view(np.uint16))


def _store16(v, dv):
    """A value v known to dv, stored as f16: (stored value of the reference, bound on |stored - kernel's stored|) where the stored
    values feed a later step.  The two roundings agree unless v lies within dv of a rounding boundary; then they differ by an f16 ulp."""
    h = r16(v)
    ulp = np.spacing(np.abs(h).astype(np.float16)).astype(np.float64)
    pow2 = np.frexp(h)[0] == 0.5   # below a power of two the spacing halves
    half = np.where(pow2 & (np.abs(v) < np.abs(h)), ulp / 4, ulp / 2)
    flip = (half - np.abs(v - h)) <= dv
    return h, np.where(flip, dv + ulp, 0.0)


# ---- attention ----------------------------------------------------------------------------------------------------------------

def attend(q, k, v, scale, p_f16=True):
    """softmax(scale q k^T) v for ONE head: q [Sq, 32], k / v [Sk, 32] -> (o [Sq, 32], bound).  No mask; exponent (s - max) scale.

    Model (bert_attention_lds_kernel / bert_attention_mfma_kernel; p_f16 = False: bert_cls_attention_kernel, whose P stays f32):
      s_ij      f32-accumulated over 32 products: ds_ij = 32 U32 sum_d |q_id k_jd|
      e_ij      (s_ij - m_i) scale: de_ij = scale (ds_ij + max_j ds_ij) + 4 U32 (|e_ij| + 1); exp itself 4 U32 relative: r_ij = de_ij + 4 U32
      P tile    f16 (U16 relative; below 2^-14, SUB16 absolute against a row sum >= 1) before P V
      P V, l    f32 accumulation over Sk keys with a rescale per 32-key block: (Sk + Sk / 16 + 8) U32 sum_j p_ij |v_jd|, twice
                (numerator and row sum); the row sum takes the unrounded p, its relative error sum_j p_ij r_ij scales |o|
      o         stored f16: U16 |o| + SUB16
    so bound_id = sum_j p_ij |v_jd| (U16 [p_f16] + r_ij) + |o_id| (sum_j p_ij r_ij + U16) + 2 acc + SUB16 (1 + sum_j |v_jd| [p_f16]):
    proportional to sum_j p_j |v_j| up to the subnormal terms."""
    q, k, v = (np.asarray(a, np.float64) for a in (q, k, v))
    sk = k.shape[0]
    s = q @ k.T
    ds = 32 * U32 * (np.abs(q) @ np.abs(k).T)
    m = s.max(axis=1, keepdims=True)
    e = (s - m) * scale
    p = np.exp(e)
    p /= p.sum(axis=1, keepdims=True)
    r = scale * (ds + ds.max(axis=1, keepdims=True)) + 4 * U32 * (np.abs(e) + 1) + 4 * U32
    o = p @ v
    spv = p @ np.abs(v)
    acc = (sk + sk / 16 + 8) * U32 * spv
    bound = (p * r) @ np.abs(v) + np.abs(o) * ((p * r).sum(axis=1, keepdims=True) + U16) + 2 * acc + SUB16
    if p_f16:
        bound = bound + U16 * spv + SUB16 * np.abs(v).sum(axis=0, keepdims=True)
    return o, bound


def attention(qkv, offsets, hidden, scale=ATTN_SCALE, cls=False):
    """qkv [T, 3H] (Q | K | V, head h at columns 32 h .. + 32), per document and head.  cls = False: ctx [T, H] (forms 0 and 1);
    cls = True: the first token of each document as the only query, ctx_cls [n_docs, H] (form 2).  Returns (ctx, bound)."""
    qkv = np.asarray(qkv, np.float64)
    n_docs = len(offsets) - 1
    out = np.zeros((n_docs if cls else qkv.shape[0], hidden))
    bound = np.zeros_like(out)
    for d in range(n_docs):
        a, b = int(offsets[d]), int(offsets[d + 1])
        if a == b:
            continue
        for h in range(hidden // 32):
            c = slice(32 * h, 32 * h + 32)
            q = qkv[a:a + 1, c] if cls else qkv[a:b, c]
            o, bd = attend(q, qkv[a:b, hidden:][:, c], qkv[a:b, 2 * hidden:][:, c], scale, p_f16=not cls)
            rows = slice(d, d + 1) if cls else slice(a, b)
            out[rows, c], bound[rows, c] = o, bd
    return out, bound


# ---- linear, GELU, LayerNorm --------------------------------------------------------------------------------------------------

def _dot(a, w, b):
    """a w^T + b with the f32-accumulation bound (K + 2) U32 (sum_k |a_k w_k| + |b|)."""
    a, w, b = (np.asarray(x, np.float64) for x in (a, w, b))
    return a @ w.T + b, (a.shape[1] + 2) * U32 * (np.abs(a) @ np.abs(w).T + np.abs(b))


def _erf_as(z):
    az = np.abs(z)
    t = 1.0 / (1.0 + 0.3275911 * az)
    poly = t * (0.2548296 + t * (-0.28449673 + t * (1.4214137 + t * (-1.453152 + t * 1.0614054))))
    return np.copysign(1.0 - poly * np.exp(-(z * z)), z)


def gelu(x):
    """x (1 + erf(x / sqrt 2)) / 2 with the Abramowitz-Stegun 7.1.26 erf of oracle.bert_oracle.gelu, in f64: the definition."""
    x = np.asarray(x, np.float64)
    return 0.5 * x * (1.0 + _erf_as(x * 0.70710678118654752440))


def _gelu_bound(x, dx, packed):
    """GELU of a value known to dx: |gelu'| dx (gelu' = Phi(x) + x phi(x), |.| <= 1.13) + the evaluation itself: 16 U32 on the erf of the
    f32 7.1.26 form (reciprocal, polynomial, exponential, 1 - . cancellation), ERF_FIT more for the packed kernels' polynomial fit."""
    grad = np.abs(0.5 * (1.0 + _erf_as(x * 0.70710678118654752440)) + x * np.exp(-0.5 * x * x) / np.sqrt(2 * np.pi)) + 1e-6
    return grad * dx + 0.5 * np.abs(x) * (16 * U32 + (ERF_FIT if packed else 0.0)) + 4 * U32 * np.abs(gelu(x))


def linear(a, w, b, epilogue=0, packed=False):
    """y = a w^T + b.  epilogue 0: f32; 1: GELU, f16; 2: f16.  packed: the fragment-order kernels (their GELU is the fitted one).
    Model: the dot-product bound; GELU through _gelu_bound; an f16 output adds U16 |y| + SUB16.  Returns (y, bound)."""
    y, dy = _dot(a, w, b)
    if epilogue == 1:
        y, dy = gelu(y), _gelu_bound(y, dy, packed)
    if epilogue:
        dy = dy + U16 * np.abs(y) + SUB16
    return y, dy


def layer_norm(y, dy, g, beta, eps=LN_EPS):
    """(y - mean) / sqrt(var + eps) g + beta over the last axis, mean and biased variance, for rows known to dy.
    Model (two passes in f32, as row_layer_norm and the GEMM epilogues): with SUMS = 12 U32 for a row sum of H terms in a fixed tree,
      mean  dmu = mean(dy) + SUMS mean|y|
      d     y - mean: dd = dy + dmu + U32 |d|
      var   dvar = 2 mean(|d| dd) + SUMS var; 1 / sqrt(var + eps) to dvar / (2 (var + eps)) + 3 U32 relative
      out   |g| inv (dd + |d| rel_inv) + 3 U32 |d inv g| + U32 |out|
    Returns (out, bound)."""
    y, dy, g, beta = (np.asarray(x, np.float64) for x in (y, dy, g, beta))
    sums = 12 * U32
    mu = y.mean(axis=-1, keepdims=True)
    dmu = dy.mean(axis=-1, keepdims=True) + sums * np.abs(y).mean(axis=-1, keepdims=True)
    d = y - mu
    dd = dy + dmu + U32 * np.abs(d)
    var = (d * d).mean(axis=-1, keepdims=True)
    dvar = 2 * (np.abs(d) * dd).mean(axis=-1, keepdims=True) + sums * var
    inv = 1.0 / np.sqrt(var + eps)
    rel_inv = dvar / (2 * (var + eps)) + 3 * U32
    out = d * inv * g + beta
    bound = np.abs(g) * inv * (dd + np.abs(d) * rel_inv) + 3 * U32 * np.abs(d * inv * g) + U32 * np.abs(out)
    return out, bound


def _with_h(out, bound):
    """(x_f32, its bound, the bound of the f16 copy against the same reference)."""
    return out, bound, bound + U16 * np.abs(out) + SUB16


def linear_ln(a, w, b, x, g, beta, eps=LN_EPS):
    """LayerNorm(x + a w^T + b): the dot-product bound plus 2 U32 (|a w^T + b| + |y|) for the two f32 additions, then layer_norm's model.
    Returns (x_f32, bound_f32, bound_h)."""
    lin, dl = _dot(a, w, b)
    y = lin + np.asarray(x, np.float64)
    return _with_h(*layer_norm(y, dl + 2 * U32 * (np.abs(lin) + np.abs(y)), g, beta, eps))


TILE_CONF = 6.0   # standard deviations at which the disagreement of two f16 tiles is carried through a projection


def ln_moments(out, g, beta):
    """(mean, second moment) per row of z = (out - beta) / g: a LayerNorm output has 0 and var / (var + eps), whatever its input was."""
    z = (np.asarray(out, np.float64) - beta) / g
    return z.mean(axis=-1), (z * z).mean(axis=-1)


def _moment_tolerances(out, y, g, beta, eps):
    """How far the moments of an f32 LayerNorm output may be from (0, var / (var + eps)), from the reference's own rows y: an element is
    dz = 4 U32 (|out| + |out - beta|) / |g| from its exact value (the three roundings of (y - mean) inv g + beta), the f32 mean is
    12 U32 mean|y| / sigma off in units of sigma, the f32 variance 15 U32 relative.  Returns (tol_mean, tol_m2, m2) per row."""
    z = (out - beta) / g
    dz = 4 * U32 * (np.abs(out) + np.abs(out - beta)) / np.abs(g)
    var = y.var(axis=-1)
    off = 12 * U32 * np.abs(y).mean(axis=-1) / np.sqrt(var + eps)
    return dz.mean(axis=-1) + off + 4 * U32, 2 * (np.abs(z) * dz).mean(axis=-1) + 2 * off * np.abs(z).mean(axis=-1) + 32 * U32, var / (var + eps)


def post_attn(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, lnw, lnb, x, eps=LN_EPS):
    """Everything of a layer after the attention (bert_ffn_w_kernel<AO>, bert_ffn_w64_kernel; or bert_gemm_ln_w_kernel followed by
    bert_ffn_w_kernel):
      x1  = LayerNorm(x + ctx w0^T + b0)     f32, kept; its f16 copy is the up-projection's operand (the x tile)
      g   = GELU(x1_h w1^T + b1)             stored f16: the intermediate tile
      out = LayerNorm(x1 + g_h w2^T + b2)    f32 and f16
    The reference rounds x1 and g to f16 where the kernels do.  Model: linear_ln's for both LayerNorms and linear's (packed GELU) for the
    up-projection.  An f16 tile element that lies within its own error of a rounding boundary may round the other way in the kernel and
    then disagrees with the reference's by one f16 ulp (_store16).  Carried through |w| element by element (every disagreement at its
    worst and of the sign that hurts), two projections deep, that alone comes to ~ 1 on outputs of ~ 1 and the test would see nothing;
    which way an element rounds depends on where its own value lies between its own two neighbours, so the disagreements of a tile
    row are taken as independent and of either sign, and their weighted sum over the row at TILE_CONF standard deviations:
    TILE_CONF sqrt(sum_c w_jc^2 e_c^2).  Every other term stays the worst-case sum.  What that leaves (~ 0.05 on outputs of ~ 1) sees a
    row or a bias in the wrong place but not a LayerNorm whose statistics are slightly off; the second LayerNorm is therefore also held
    to its invariant, which no earlier error touches: (out - ln_b) / ln_w has mean 0 and second moment var / (var + eps) per row
    (ln_moments), to the tolerances of _moment_tolerances.
    Returns (x_f32, bound_f32, bound_h, (tol_mean, tol_m2, m2))."""
    w1, w2 = np.asarray(w1, np.float64), np.asarray(w2, np.float64)
    x1, dx1, _ = linear_ln(ctx, w0, b0, x, ln0w, ln0b, eps)
    x1h, dx1h = _store16(x1, dx1)
    u, du = _dot(x1h, w1, b1)
    du = du + TILE_CONF * np.sqrt((dx1h * dx1h) @ (w1 * w1).T)
    gh, dgh = _store16(gelu(u), _gelu_bound(u, du, True))
    lin, dl = _dot(gh, w2, b2)
    dl = dl + TILE_CONF * np.sqrt((dgh * dgh) @ (w2 * w2).T)
    y = lin + x1
    out, bound, bound_h = _with_h(*layer_norm(y, dl + dx1 + 2 * U32 * (np.abs(lin) + np.abs(y)), lnw, lnb, eps))
    return out, bound, bound_h, _moment_tolerances(out, y, np.asarray(lnw, np.float64), np.asarray(lnb, np.float64), eps)


def embed_ln(ids, positions, types, word, pos, type_emb, g, beta, eps=LN_EPS):
    """LayerNorm((word[id] + pos[p]) + type[t]): two f32 additions, U32 (|word + pos| + |v|), then layer_norm's model.
    Returns (x_f32, bound_f32, bound_h)."""
    word, pos, type_emb = (np.asarray(a, np.float64) for a in (word, pos, type_emb))
    wp = word[ids] + pos[positions]
    v = wp + type_emb[types]
    return _with_h(*layer_norm(v, U32 * (np.abs(wp) + np.abs(v)), g, beta, eps))


def pool(x, offsets):
    """Mean over a document's tokens, then L2; a squared norm at or below f32::EPSILON (or an empty document) gives zeros, exactly.
    Model (bert_pool_kernel): the mean to (n / 16 + 20) U32 mean|x| (sixteen partial rows, each a chain of n / 16 additions, added in
    order; the division), the squared norm to 2 sum |val| dval + 24 U32 norm_sq, its inverse root to half of that + 3 U32 relative.
    Returns (out [n_docs, H], bound)."""
    x = np.asarray(x, np.float64)
    n_docs = len(offsets) - 1
    out = np.zeros((n_docs, x.shape[1]))
    bound = np.zeros_like(out)
    for d in range(n_docs):
        a, b = int(offsets[d]), int(offsets[d + 1])
        if a == b:
            continue
        n = b - a
        val = x[a:b].sum(axis=0) / n
        dval = (n / 16 + 20) * U32 * np.abs(x[a:b]).sum(axis=0) / n
        nsq = float((val * val).sum())
        dnsq = 2 * float((np.abs(val) * dval).sum()) + 24 * U32 * nsq
        assert abs(nsq - POOL_GUARD) > 4 * dnsq, "test input sits on the zero guard"
        if nsq <= POOL_GUARD:
            continue
        s = 1.0 / np.sqrt(nsq)
        out[d] = val * s
        bound[d] = dval * s + np.abs(out[d]) * (dnsq / (2 * nsq) + 4 * U32)
    return out, bound


# ---- the inputs of the stage tests (tests/test_gpu_encoder_stages.py; the contract test mutates references on the same ones) ------

ATTN_LENGTHS = [1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 449, 505, 506, 511, 512]
ATTN_FAMILIES = ["needle", "uniform", "trained"]
NEEDLE_PLACES = [0, 15, 16, 31, 32, -2, -1]


def attention_ragged(heads, cls=False):
    """Document lengths of the multi-document calls: empty documents at the start, in the middle and at the end (none for the [CLS]
    form, which takes no empty document); max_seq > 128 with n_docs heads < 512 (two blocks per document and head in the f16 form);
    n_docs heads >= 512 with one document of 200 tokens; one long document among many of one token (waves that leave at once)."""
    many = -(-512 // heads) + 3
    calls = [[0, 200, 0, 33, 1, 64, 17, 0],
             [0, 3] + [200] + [1 + (i * 5) % 9 for i in range(many - 5)] + [0, 2, 0],
             [1] * 20 + [300] + [1] * 20]
    calls = [c for c in calls]
    assert calls[0] and max(calls[0]) > 128 and len(calls[0]) * heads < 512 and len(calls[1]) * heads >= 512
    return [[n for n in c if n or not cls] for c in calls]


def attention_inputs(family, lens, hidden, seed, rot=0):
    """qkv [T, 3H] of f16-representable f32 for documents of `lens` tokens.
      needle   per head one key whose score dominates for every query of the document (p ~ 1): its V row is +1, every other V row -1;
               head h has it at NEEDLE_PLACES[(h + rot) % 7] (0, 15, 16, 31, 32, S - 2, S - 1, clipped into the document)
      uniform  Q = 0: every output row is the mean of the document's V rows; V[S - 1] is 64 x the rest and every other document's V rows
               are 64 x larger than its neighbours', so a clamped padding key or a neighbour's key moves the mean
      trained  logits of standard deviation ~ 4 after scaling (q, k ~ 2 N(0, 1)), Student-t (3 degrees of freedom) values"""
    rng = np.random.default_rng(seed)
    heads, total = hidden // 32, int(sum(lens))
    q = np.zeros((total, hidden))
    k = np.zeros((total, hidden))
    v = np.zeros((total, hidden))
    t0 = 0
    for di, s in enumerate(lens):
        sl = slice(t0, t0 + s)
        t0 += s
        if s == 0:
            continue
        if family == "needle":
            k[sl] = rng.choice([-1.0, 1.0], (s, hidden))
            v[sl] = -1.0
            for h in range(heads):
                place = NEEDLE_PLACES[(h + rot + di) % len(NEEDLE_PLACES)]
                place = min(place, s - 1) if place >= 0 else max(s + place, 0)
                c = slice(32 * h, 32 * h + 32)
                q[sl, c] = 12.0 * k[t0 - s + place, c] + rng.integers(-1, 2, (s, 32))
                v[t0 - s + place, c] = 1.0
        elif family == "uniform":
            k[sl] = rng.standard_normal((s, hidden))
            v[sl] = rng.standard_normal((s, hidden)) * (64.0 if di % 2 else 1.0)
            v[t0 - 1] *= 64.0
        else:
            q[sl] = 2.0 * rng.standard_normal((s, hidden))
            k[sl] = 2.0 * rng.standard_normal((s, hidden))
            v[sl] = rng.standard_t(3, (s, hidden))
    return h16(np.concatenate([q, k, v], axis=1))


def offsets_of(lens):
    return np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)


UNIQUE_ROWS = 257   # rows of a large-M input repeat with this period: prime, so a row taken a tile (16 / 32 / 64 rows) away is another row


def tile_rows(u, m):
    """m rows out of the unique rows u (row i = u[i % len(u)]): the reference of a many-thousand-row call costs that of len(u) rows."""
    return u[np.arange(m) % u.shape[0]]


def linear_inputs(n, k, seed):
    """a [257, k] (tile_rows gives a call its m rows) with row i scaled by 1 + i mod 7 (a row landing in the wrong place shows), w [n, k], bias [n]."""
    rng = np.random.default_rng(seed)
    rows = UNIQUE_ROWS
    a = rng.standard_normal((rows, k)) * (1 + np.arange(rows) % 7)[:, None]
    return h16(a), h16(rng.standard_normal((n, k)) * 0.05), (rng.standard_normal(n) * 0.1).astype(np.float32)


def ln_params(hidden, rng):
    return (1.0 + 0.1 * rng.standard_normal(hidden)).astype(np.float32), (0.05 * rng.standard_normal(hidden)).astype(np.float32)


def linear_ln_inputs(hidden, k, seed):
    """a, w, bias, x, ln_w, ln_b.  The residual x is chosen so that x + a w^T + bias has, by row: i % 5 == 3 a standard deviation of ~ 1e-3
    around 0, i % 5 == 4 a mean of 50 against a standard deviation of 0.5 (|mean| >> sigma), otherwise N(0, 1); rows i % 5 == 1 have a small
    projection (a scaled by 2^-10), so that their bound is the LayerNorm's own and not the dot product's."""
    rng = np.random.default_rng(seed)
    rows = UNIQUE_ROWS
    i = np.arange(rows)
    a = h16(rng.standard_normal((rows, k)) * np.where(i % 5 == 1, 2.0 ** -10, 1.0)[:, None])
    w = h16(rng.standard_normal((hidden, k)) * 0.05)
    b = (rng.standard_normal(hidden) * 0.1).astype(np.float32)
    target = rng.standard_normal((rows, hidden))
    target[i % 5 == 3] *= 1e-3
    target[i % 5 == 4] = 50.0 + 0.5 * target[i % 5 == 4]
    x = (target - (a.astype(np.float64) @ w.astype(np.float64).T + b)).astype(np.float32)
    g, beta = ln_params(hidden, rng)
    return a, w, b, x, g, beta


def post_attn_inputs(hidden, inter, seed):
    """ctx, w0, b0, ln0_w, ln0_b, w1, b1, w2, b2, ln_w, ln_b, x: weights at the scale of oracle.bert_oracle.random_weights, biases
    of ~ 0.5 (one that lands 16 columns off shows), the context with row i scaled by 1 + i mod 3."""
    rng = np.random.default_rng(seed)
    rows = UNIQUE_ROWS
    ctx = h16(rng.standard_normal((rows, hidden)) * (1 + np.arange(rows) % 3)[:, None])
    w0 = h16(rng.standard_normal((hidden, hidden)) * 0.05)
    b0 = (rng.standard_normal(hidden) * 0.5).astype(np.float32)
    ln0w, ln0b = ln_params(hidden, rng)
    w1 = h16(rng.standard_normal((inter, hidden)) * 0.05)
    b1 = (rng.standard_normal(inter) * 0.5).astype(np.float32)
    w2 = h16(rng.standard_normal((hidden, inter)) * 0.05)
    b2 = (rng.standard_normal(hidden) * 0.5).astype(np.float32)
    lnw, lnb = ln_params(hidden, rng)
    x = rng.standard_normal((rows, hidden)).astype(np.float32)
    return ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, lnw, lnb, x


def embed_inputs(tokens, hidden, seed, vocab=50, max_pos=512):
    """ids (0 and vocab - 1 among them), positions (0 and 511 among them), types (both), word, pos, type [2, H], ln_w, ln_b."""
    rng = np.random.default_rng(seed)
    ids = rng.integers(0, vocab, tokens).astype(np.int32)
    positions = rng.integers(0, max_pos, tokens).astype(np.int32)
    types = (np.arange(tokens) % 2).astype(np.int32)
    ids[0], positions[0] = 0, 0
    ids[-1], positions[-1] = vocab - 1, max_pos - 1
    if tokens > 2:
        ids[1], positions[1] = vocab - 1, 0
        ids[2], positions[2] = 0, max_pos - 1
    word = (rng.standard_normal((vocab, hidden)) * 0.5).astype(np.float32)
    pos = (rng.standard_normal((max_pos, hidden)) * 0.1).astype(np.float32)
    type_emb = (rng.standard_normal((2, hidden)) * 0.1).astype(np.float32)
    g, beta = ln_params(hidden, rng)
    return ids, positions, types, word, pos, type_emb, g, beta


POOL_LENS = [0, 1, 15, 16, 17, 512, 3, 0]   # document 6 (3 tokens): rows of ~ 1e-6, its mean is below the zero guard


def pool_inputs(hidden, seed):
    rng = np.random.default_rng(seed)
    offsets = offsets_of(POOL_LENS)
    x = rng.standard_normal((int(offsets[-1]), hidden)).astype(np.float32)
    x[offsets[6]:offsets[7]] *= np.float32(1e-6)
    return x, offsets


# ---- the lab entry point --------------------------------------------------------------------------------------------------------

def run_stage(stage, form, ins, out_shapes, offsets=None, ids=None, positions=None, types=None, expect=0, **scalars):
    """fsgpu_lab_bert_stage on host arrays: ins = the f32 inputs in the header's order, out_shapes = shapes of out0 (and out1).
    Returns the outputs (f32), or the status when it is not `expect`ed to be FSGPU_OK."""
    from frankensearch_amd import _lib
    a = _lib.BertStageArgs()
    a.stage, a.form = stage, form
    for name, value in scalars.items():
        setattr(a, name, value)
    keep = [np.ascontiguousarray(x, np.float32) for x in ins]
    for i, x in enumerate(keep):
        a.in_[i] = x.ctypes.data
    for name, arr, dtype in (("offsets", offsets, np.uint32), ("ids", ids, np.int32), ("positions", positions, np.int32), ("types", types, np.int32)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype)
            keep.append(arr)
            setattr(a, name, arr.ctypes.data)
    outs = [np.full(shape, np.nan, np.float32) for shape in out_shapes]
    a.out0 = outs[0].ctypes.data
    if len(outs) > 1:
        a.out1 = outs[1].ctypes.data
    import ctypes
    status = _lib.lib().fsgpu_lab_bert_stage(0, ctypes.byref(a))
    if expect != 0 or status != 0:
        assert status == expect, (status, _lib.last_error())
        return status
    return outs

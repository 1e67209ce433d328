"""References of the int8 encoder's launches (bert_int8.hip) and of the cross-encoder's head (bert_cls_head_kernel), the
inputs of tests/test_gpu_int8_stages.py, and the two lab entry points as Python calls.  Test helper, not collected; imports without a GPU.

Exact parts (bits are compared): the quantiser's codes and scales (int8_dynamic_ref.quantize_rows of the operand the kernel saw), the
packed weight bytes (pack_w: the fragment order as an index formula), the GEMM with the bias epilogue (gemm_exact).
Bounded parts (encoder_stage_ref.compare against a bound derived from the reference's own f64 intermediates): the GELU epilogue (the
pre-activation is the exact epilogue-0 value, so the bound is the evaluation's alone), the f32 rows of the two LayerNorm-quantisers
(their codes and scale are again exact: the quantisation of the f32 row the kernel itself stored), and the head.

Pass condition of a bounded part: ratio <= SAFETY[stage]; the factors follow the rule of encoder_stage_ref (at most 4, the largest ratio
measured on an MI355X at most half of the factor, an f32 output that measures under 0.5 held to the bare bound): profiles/int8_stages/ratios.txt.
"""
import numpy as np

import encoder_stage_ref as E
import int8_dynamic_ref as Q

F = np.float32
U32 = E.U32
TINY32 = float(np.finfo(np.float32).tiny)   # the smallest normal f32: a sigmoid below it may come back as 0
LN_EPS = E.LN_EPS

QUANT_ROWS, PACK_W, GEMM, EMBED_LN_QUANT, ADD_LN_QUANT = range(5)
CLS_HEAD = 6   # of fsgpu_lab_bert_stage

# tanhf and expf are library functions: the OpenCL full-profile limits their implementation is written to are 5 ulp (tanh) and 3 ulp
# (exp), an ulp being 2 U32.  The sigmoid adds one f32 addition and one IEEE division to its exponential.
TANH_U = 10 * U32
SIGMOID_U = (6 + 2) * U32

# Measured on an MI355X (profiles/int8_stages/ratios.txt): every f32 output under 0.5 and held to the bare bound, except the embedding:
# its row of standard deviation 1e-3 is the sum of a word and a position row of ~ 0.1 that cancel, so the two roundings of those f32
# additions ARE its error and the bound of them is tight (0.70 measured; numpy's f32 evaluation of the same row gives the same 0.70).
SAFETY = {"gemm_gelu": 1.0, "embed_ln_quant": 2.0, "add_ln_quant": 1.0, "cls_head": 1.0}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a.view(np.uint8)


# ---- exact restatements ---------------------------------------------------------------------------------------------------------------

def pack_index(n_rows, k_cols):
    """Where code (n, k) of a [N, K] weight lies among the N K packed bytes: tile (n >> 4) (K >> 6) + (k >> 6) of 64 lanes x 16 bytes,
    lane (n & 15) + 16 ((k & 63) >> 4), byte k & 15."""
    n = np.arange(n_rows)[:, None]
    k = np.arange(k_cols)[None, :]
    tile = (n >> 4) * (k_cols >> 6) + (k >> 6)
    lane = (n & 15) + 16 * ((k & 63) >> 4)
    return (tile * 64 + lane) * 16 + (k & 15)


def pack_w(w, index=pack_index):
    """(packed bytes int8 [N K], sw f32 [N]) of launch_bert_i8_pack_w."""
    q, s = Q.quantize_rows(w)
    out = np.zeros(q.size, np.int8)
    out[index(*q.shape).ravel()] = q.ravel()
    return out, s


def gemm_exact(codes, sa, w, bias):
    """y f32 [M, N] of the bias epilogue: ((float)acc (sa[m] sw[n])) + b[n], acc exact."""
    qw, sw = Q.quantize_rows(w)
    acc = Q.int_matmul(np.asarray(codes, np.int8), qw)
    scale = (np.asarray(sa, F)[:, None] * sw[None, :]).astype(F)
    return ((acc.astype(F) * scale).astype(F) + np.asarray(bias, F)[None, :]).astype(F)


# ---- bounded references -----------------------------------------------------------------------------------------------------------------

def gemm_gelu(codes, sa, w, bias):
    """(GELU of the exact pre-activation in f64, bound of the f32 evaluation alone)."""
    pre = gemm_exact(codes, sa, w, bias).astype(np.float64)
    return E.gelu(pre), E._gelu_bound(pre, 0.0, packed=False)


def embed_ln(ids, positions, word, pos, type0, g, beta, eps=LN_EPS):
    """LayerNorm((word[id] + pos[p]) + type0) -> (x, bound): encoder_stage_ref.embed_ln with token type 0 throughout."""
    out, bound, _ = E.embed_ln(ids, positions, np.zeros(len(ids), np.int64), word, pos, np.asarray(type0).reshape(1, -1), g, beta, eps)
    return out, bound


def add_ln(x, delta, g, beta, eps=LN_EPS):
    """LayerNorm(x + delta) -> (x, bound): one f32 addition (U32 |x + delta|), then encoder_stage_ref.layer_norm's model."""
    y = np.asarray(x, np.float64) + np.asarray(delta, np.float64)
    return E.layer_norm(y, U32 * np.abs(y), g, beta, eps)


def _sigmoid(x):
    with np.errstate(over="ignore"):
        return 1.0 / (1.0 + np.exp(-x))


def cls_head(x_cls, pool_w, pool_b, cls_w, cls_b, tanh=np.tanh, sign=1.0):
    """pooled = tanh(W_p cls + b_p), logit = w_c . pooled + b_c, score = sigmoid(logit) -> (logit, dlogit, score, dscore) per pair.
      pre     the f32 dot-product bound (_dot)
      pooled  sech^2 at the point of |pre| +- dpre nearest 0, times dpre, plus TANH_U |pooled|
      logit   sum |w_c| dpooled plus the dot-product bound of the classifier row
      score   sigma' at the point of |logit| +- dlogit nearest 0, times dlogit, plus SIGMOID_U sigma, plus TINY32 (a score that
              underflows comes back as 0)
    A row with a NaN or an Inf gives a non-finite logit; the test holds such a pair to score 0.0 and leaves it out of the comparison.
    `tanh` and `sign` exist for the contract test's mutations."""
    with np.errstate(invalid="ignore", over="ignore"):
        cls_w = np.asarray(cls_w, np.float64).reshape(-1)
        b_c = float(np.asarray(cls_b).reshape(-1)[0])
        pre, dpre = E._dot(x_cls, pool_w, pool_b)
        pooled = tanh(pre)
        near = np.maximum(np.abs(pre) - dpre, 0.0)
        dpooled = (1.0 - np.tanh(near) ** 2) * dpre + TANH_U * np.abs(pooled)
        logit = pooled @ cls_w + b_c
        dlogit = dpooled @ np.abs(cls_w) + (cls_w.size + 2) * U32 * (np.abs(pooled) @ np.abs(cls_w) + abs(b_c))
        score = _sigmoid(sign * logit)
        s_near = _sigmoid(np.maximum(np.abs(logit) - dlogit, 0.0))
        dscore = s_near * (1.0 - s_near) * dlogit + SIGMOID_U * score + TINY32
    return logit, dlogit, score, dscore


# ---- inputs of the stage tests ---------------------------------------------------------------------------------------------------------------

QUANT_ROW_COUNTS = [1, 3, 4, 5, 33]
QUANT_KS = [64, 128, 384, 1280, 1536, 4096]
QUANT_FAMILIES = ["gauss", "zero_row", "one_hot", "outlier", "ties", "rust_pin", "amax_3e38", "tiny_amax"]
QUANT_FAMILIES_F16 = ["gauss", "zero_row", "one_hot", "outlier", "ties", "rust_pin", "f16_subnormal", "f16_max", "below_f16"]


def quant_inputs(family, rows, k, seed):
    """[rows, k] f32.  The special row of a family is the LAST one (the only one of a one-row call)."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((rows, k)).astype(F)
    j = np.arange(k)
    if family == "zero_row":
        x[-1] = 0.0
    elif family == "one_hot":
        x[-1] = 0.0
        x[-1, k - 7] = -0.3
    elif family == "outlier":
        x[:, [0, k - 1]] *= F(1000.0)
    elif family == "ties":
        # amax = 127 exactly (inv = 1): every other entry +-(i + 0.5), an exact tie of either sign
        x[-1] = ((j % 126) + 0.5) * np.where(j % 2 == 0, 1.0, -1.0)
        x[-1, k // 2] = 127.0
    elif family == "rust_pin":
        pin = np.zeros((4, k), F)
        pin[:, :8] = Q.rust_quant_pin_matrix()
        x = pin[np.arange(rows) % 4]
    elif family == "amax_3e38":
        x = (x / np.max(np.abs(x), axis=1, keepdims=True) * F(3.0e38)).astype(F)
    elif family == "tiny_amax":
        # 127 / amax overflows below 127 / FLT_MAX ~ 3.73e-37: rows on either side of it, a subnormal one among them
        for r in range(rows):
            a = F([1e-38, 3.0e-37, 1e-42, 4.0e-37, 3.8e-37][(r + rows) % 5])
            x[r] = np.where(j % 2 == 0, a, F(0.0)) * np.where(j % 4 == 0, F(1.0), F(-1.0))
            x[r, 5] = a * F(0.03)
    elif family == "f16_subnormal":
        x[-1] = (j % 37) * 2.0 ** -24 * np.where(j % 2 == 0, 1.0, -1.0)      # amax 36 x 2^-24, zeros among them
    elif family == "f16_max":
        x[-1, [3, k - 2]] = [65504.0, -65504.0]
    elif family == "below_f16":
        # neighbours that differ only below f16 precision: 1 + i 2^-14 for i in 0..7 round (to even) to 1, 1, 1 + 2^-10 ... in f16
        x[-1] = (1.0 + (j % 8) * 2.0 ** -14) * np.where(j % 3 == 0, -1.0, 1.0)
        x[-1, 0] = 1.0 + 2.0 ** -10
    else:
        assert family == "gauss", family
    return np.ascontiguousarray(x, F)


PACK_SHAPES = [(64, 64), (192, 128), (384, 384), (1536, 384), (384, 1536)]


def pack_inputs(n, k, seed):
    """w [n, k]: an all-zero channel, a one-hot channel, outlier input channels."""
    rng = np.random.default_rng(seed)
    w = (rng.standard_normal((n, k)) * 0.05).astype(F)
    w[:, [1, k // 2]] *= F(1000.0)
    w[3] = 0.0
    w[5] = 0.0
    w[5, k - 7] = -0.3
    return w


GEMM_MS = [1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 97, 129]
GEMM_NS = [64, 128, 192, 384]
GEMM_KS = [64, 128, 384, 1536]


def gemm_shapes():
    """Every M at (N, K) = (192, 128), every (N, K) at M in {1, 33, 65}."""
    shapes = [(m, 192, 128) for m in GEMM_MS]
    shapes += [(m, n, k) for n in GEMM_NS for k in GEMM_KS for m in (1, 33, 65) if (m, n, k) not in shapes]
    return shapes


def gemm_inputs(family, m, n, k, seed):
    """codes int8 [m, k], sa f32 [m], w f32 [n, k], bias f32 [n].
      random      codes over the whole range, a weight with a zero and a one-hot channel
      sa_zero     the first and the last row have scale 0: their outputs are the bias
      extreme     K = 4096 by intent: every activation code +-127, every weight code +-127: |acc| = 66,064,384 > 2^24
      extreme_odd the same with the first (row % 61) activation codes at 126 and the first (channel % 29) weight codes at 126, so that
                  the accumulators above 2^24 take every residue and (float)acc must round (to nearest, ties to even)
      cancel      alternating +-127 against constant channels: every accumulator is 0
      gelu_sweep  K = 64 by intent: zero codes, the bias sweeps [-12, 12] with +0 and -0: the pre-activation is the bias"""
    rng = np.random.default_rng(seed)
    codes = rng.integers(-127, 128, (m, k)).astype(np.int8)
    sa = (np.abs(rng.standard_normal(m)) * 0.02 + 0.001).astype(F)
    w = (rng.standard_normal((n, k)) * 0.05).astype(F)
    bias = (rng.standard_normal(n) * 0.1).astype(F)
    if family == "random":
        w[3] = 0.0
        w[5] = 0.0
        w[5, k - 7] = -0.3
    elif family == "sa_zero":
        sa[[0, -1]] = 0.0
    elif family in ("extreme", "extreme_odd"):
        row_sign = np.where(np.arange(m) % 2 == 0, 127, -127)
        codes = np.repeat(row_sign[:, None], k, axis=1).astype(np.int8)
        w = np.repeat(np.where(np.arange(n) % 3 == 0, -0.3, 0.3)[:, None], k, axis=1).astype(F)
        if family == "extreme_odd":
            for r in range(m):
                codes[r, :r % 61] = np.sign(codes[r, 0]) * 126
            for c in range(n):
                w[c, :c % 29] *= F(126.0 / 127.0)
        sa[:] = F(0.02)
    elif family == "cancel":
        codes = np.repeat(np.where(np.arange(k) % 2 == 0, 127, -127)[None, :], m, axis=0).astype(np.int8)
        w = np.repeat((0.01 * (1 + np.arange(n) % 5))[:, None], k, axis=1).astype(F)
    elif family == "gelu_sweep":
        codes[:] = 0
        bias = np.concatenate([np.linspace(-12.0, 12.0, n - 2), [0.0, -0.0]]).astype(F)
    else:
        raise AssertionError(family)
    return codes, sa, w, bias


LN_HIDDEN = [64, 128, 384, 768, 1024]
LN_TOKENS = [1, 3, 4, 5, 9]


def ln_rows(tokens, hidden, rng):
    """The row families of encoder_stage_ref.linear_ln_inputs: token 0 has a standard deviation of 1e-3 around 0, token 1 a mean of 50
    against a standard deviation of 0.5, the others are N(0, 1)."""
    target = rng.standard_normal((tokens, hidden))
    target[0] *= 1e-3
    if tokens > 1:
        target[1] = 50.0 + 0.5 * target[1]
    return target


def add_ln_inputs(tokens, hidden, seed):
    """x, delta, ln_w, ln_b with x + delta = ln_rows."""
    rng = np.random.default_rng(seed)
    delta = (rng.standard_normal((tokens, hidden)) * 0.5).astype(F)
    x = (ln_rows(tokens, hidden, rng) - delta).astype(F)
    g, beta = E.ln_params(hidden, rng)
    return x, delta, g, beta


def embed_inputs(tokens, hidden, seed, vocab=50, max_pos=512):
    """ids, positions, word, pos, type0, ln_w, ln_b: encoder_stage_ref.embed_inputs (ids 0 and vocab - 1, positions 0 and max_pos - 1
    among them) with word row 0 such that (id 0, position 0) sums to a row of standard deviation 1e-3 and word row vocab - 1 at a mean
    of 50 against a standard deviation of 0.5."""
    ids, positions, _, word, pos, type_emb, g, beta = E.embed_inputs(tokens, hidden, seed, vocab, max_pos)
    rng = np.random.default_rng(seed + 1)
    word[0] = (1e-3 * rng.standard_normal(hidden) - pos[0].astype(np.float64) - type_emb[0]).astype(F)
    word[vocab - 1] = (50.0 + 0.5 * rng.standard_normal(hidden)).astype(F)
    return ids, positions, word, pos, type_emb[0].copy(), g, beta


HEAD_HIDDEN = [64, 128, 384, 1024]
HEAD_PAIRS = [1, 2, 17]
HEAD_BIASES = [-110.0, -104.5, -97.0, -90.5, 90.5, 97.0, 104.5, 110.0]


def head_inputs(family, pairs, hidden, seed, cls_b=None):
    """x_cls [pairs, hidden], pool_w, pool_b, cls_w [hidden], cls_b [1].
      ordinary   the scales of reranker_ref.head_weights
      saturated  pooler rows scaled so that |pre| reaches ~ 30: tanh is +-1 to the last bit for most outputs
      extreme    a small classifier row and a bias `cls_b` beyond +-90 / +-104: exp(-logit) underflows or overflows"""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((pairs, hidden)).astype(F)
    pool_w = (rng.standard_normal((hidden, hidden)) / np.sqrt(hidden)).astype(F)
    pool_b = (rng.standard_normal(hidden) * 0.05).astype(F)
    w_c = (rng.standard_normal(hidden) * 4.0 / np.sqrt(hidden)).astype(F)
    b_c = (rng.standard_normal(1) * 0.1).astype(F)
    if family == "saturated":
        pool_w = (pool_w * np.linspace(0.5, 13.0, hidden)[:, None]).astype(F)
    elif family == "extreme":
        w_c = (w_c * F(0.02)).astype(F)
        b_c = np.array([cls_b], F)
    else:
        assert family == "ordinary", family
    return x, pool_w, pool_b, w_c, b_c


# ---- the lab entry points -----------------------------------------------------------------------------------------------------------------------

def run_int8_stage(stage, form=0, ins=(), codes=None, ids=None, positions=None, f32_shape=None, q_shape=None, s_len=None, expect=0,
                   **scalars):
    """fsgpu_lab_bert_int8_stage on host arrays: ins = the f32 inputs in the header's order.  Returns {"x": f32 output, "q": codes,
    "s": scales [s_len, or q_shape[0]]} (those the stage has), or the status when it is not `expect`ed to be FSGPU_OK."""
    import ctypes
    from frankensearch_amd import _lib
    a = _lib.BertInt8StageArgs()
    a.stage, a.form = stage, form
    for name, value in scalars.items():
        setattr(a, name, value)
    keep = [np.ascontiguousarray(x, F) for x in ins]
    for i, x in enumerate(keep):
        a.in_[i] = x.ctypes.data
    for name, arr, dtype in (("codes", codes, np.int8), ("ids", ids, np.int32), ("positions", positions, np.int32)):
        if arr is not None:
            arr = np.ascontiguousarray(arr, dtype)
            keep.append(arr)
            setattr(a, name, arr.ctypes.data)
    out = {}
    if f32_shape is not None:
        out["x"] = np.full(f32_shape, np.nan, F)
        a.out_f32 = out["x"].ctypes.data
    if q_shape is not None:
        out["q"] = np.full(q_shape, 0x55, np.int8)
        out["s"] = np.full(q_shape[0] if s_len is None else s_len, np.nan, F)
        a.out_codes, a.out_scales = out["q"].ctypes.data, out["s"].ctypes.data
    status = _lib.lib().fsgpu_lab_bert_int8_stage(0, ctypes.byref(a))
    if expect != 0 or status != 0:
        assert status == expect, (status, _lib.last_error())
        return status
    return out


def run_pack(w):
    n, k = w.shape
    return run_int8_stage(PACK_W, 0, [w], q_shape=(n * k,), s_len=n, n=n, k=k)


def run_head(x_cls, pool_w, pool_b, cls_w, cls_b, expect=0):
    """The CLS_HEAD stage of fsgpu_lab_bert_stage: (logits [m], scores [m])."""
    m, hidden = x_cls.shape
    out = E.run_stage(CLS_HEAD, 0, [x_cls, pool_w, pool_b, cls_w, cls_b], [(m,), (m,)], m=m, hidden=hidden, expect=expect)
    return out

"""numpy restatement of the int8 dynamic-quant linear contract (FSGPU_BERT_LINEAR_INT8_DYNAMIC).  Test helper, not
collected.

Per row (a weight's output channel, or a row of a linear's input):
    amax = max |x|;  inv = 127.0f / amax;  q = clamp(round_half_away(x * inv), -127, 127);  scale = amax / 127.0f
    an all-zero row: q = 0, scale = 0.  Both divisions and the product are IEEE f32.
    a row with 0 < amax < 127 / FLT_MAX has inv = +inf: its zeros code to 0, its other elements to +-127.
Linear:  acc = sum_k qx * qw (exact);  y = ((float)acc * (sx[m] * sw[n])) + b[n], each an f32 operation.

The quotient x * inv is formed in f32 and rounded half away from zero in f64 (exact: |x * inv| < 2^8 has at most 24 significant
bits), because trunc(v + 0.5) in f32 mis-rounds 0.49999997.  The accumulation runs as an f64 matrix product, exact because every
partial sum is an integer below 127 * 127 * K < 2^53 — the int64 result is the i32 one."""
from __future__ import annotations

from typing import Dict, Sequence

import numpy as np

F = np.float32


def round_half_away(v: np.ndarray) -> np.ndarray:
    """Rust's f32::round: ties away from zero.  In f64, where v + 0.5 is exact for an f32 v."""
    v = np.asarray(v, dtype=np.float64)
    return np.copysign(np.floor(np.abs(v) + 0.5), v)


def quantize_rows(x: np.ndarray):
    """[R, K] f32 -> (codes int8 [R, K], scales f32 [R])."""
    x = np.ascontiguousarray(x, dtype=F)
    amax = np.max(np.abs(x), axis=1) if x.shape[1] else np.zeros(x.shape[0], F)
    q = np.zeros(x.shape, np.int8)
    s = np.zeros(x.shape[0], F)
    nz = amax > 0
    if np.any(nz):
        # 0 < amax < 127 / FLT_MAX: inv = +inf (the tiny-amax rule): a non-zero element goes to +-inf and codes to +-127, a zero stays 0
        with np.errstate(over="ignore", invalid="ignore"):
            inv = (F(127.0) / amax[nz]).astype(F)
            v = np.where(x[nz] == 0, F(0.0), (x[nz] * inv[:, None]).astype(F))
        q[nz] = np.clip(round_half_away(v), -127, 127).astype(np.int8)
        s[nz] = (amax[nz] / F(127.0)).astype(F)
    return q, s


def int_matmul(qx: np.ndarray, qw: np.ndarray) -> np.ndarray:
    """qx [M, K] int8 x qw [N, K]^T -> exact int64 [M, N]."""
    assert 127 * 127 * qx.shape[1] < 2 ** 53
    return (qx.astype(np.float64) @ qw.astype(np.float64).T).astype(np.int64)


def linear_int8_dynamic(x: np.ndarray, w: np.ndarray, b: np.ndarray) -> np.ndarray:
    """y [M, N] f32 of the contract: the bits fsgpu_lab_linear_int8_dynamic must return."""
    qx, sx = quantize_rows(x)
    qw, sw = quantize_rows(w)
    acc = int_matmul(qx, qw)
    scale = (sx[:, None] * sw[None, :]).astype(F)
    return ((acc.astype(F) * scale).astype(F) + np.asarray(b, F)[None, :]).astype(F)


def embed_forward_int8(weights: Dict[str, np.ndarray], batch: Sequence[Sequence[int]], num_layers: int,
                       ctx_from_f16: bool = True) -> np.ndarray:
    """oracle.bert_oracle.embed_forward with only the linears replaced by linear_int8_dynamic (Q/K/V as ONE [3H, H] linear, as
    native.rs:1546-1600 fuses them).  ctx_from_f16: the attention context is rounded to f16 before it is quantised, as the GPU's
    int8 mode quantises it from the f16 context the attention kernel writes."""
    from oracle import bert_oracle as bo

    w = bo.normalise_keys(weights)
    hidden = w["bert.embeddings.word_embeddings.weight"].shape[1]
    scale = F(0.17677669)
    lens = [len(ids) for ids in batch]
    out = np.zeros((len(batch), hidden), dtype=F)
    if sum(lens) == 0:
        return out
    ids_flat = np.concatenate([np.asarray(ids, dtype=np.int64) for ids in batch if len(ids)])
    pos_flat = np.concatenate([np.arange(n, dtype=np.int64) for n in lens if n])
    x = (w["bert.embeddings.word_embeddings.weight"][ids_flat] + w["bert.embeddings.position_embeddings.weight"][pos_flat]).astype(F)
    x = bo.layer_norm(x + w["bert.embeddings.token_type_embeddings.weight"][0], w["bert.embeddings.LayerNorm.weight"],
                      w["bert.embeddings.LayerNorm.bias"])
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(int)
    for layer in range(num_layers):
        p = f"bert.encoder.layer.{layer}"
        wq = np.concatenate([w[f"{p}.attention.self.{n}.weight"] for n in ("query", "key", "value")], axis=0)
        bq = np.concatenate([w[f"{p}.attention.self.{n}.bias"] for n in ("query", "key", "value")], axis=0)
        qkv = linear_int8_dynamic(x, wq, bq)
        ctx = np.zeros_like(x)
        for d, n in enumerate(lens):
            if n:
                a, b = offsets[d], offsets[d + 1]
                ctx[a:b] = bo.attention(qkv[a:b], hidden, scale)
        if ctx_from_f16:
            ctx = ctx.astype(np.float16).astype(F)
        attn = linear_int8_dynamic(ctx, w[f"{p}.attention.output.dense.weight"], w[f"{p}.attention.output.dense.bias"])
        x = bo.layer_norm(x + attn, w[f"{p}.attention.output.LayerNorm.weight"], w[f"{p}.attention.output.LayerNorm.bias"])
        inter = bo.gelu(linear_int8_dynamic(x, w[f"{p}.intermediate.dense.weight"], w[f"{p}.intermediate.dense.bias"]))
        ffn = linear_int8_dynamic(inter, w[f"{p}.output.dense.weight"], w[f"{p}.output.dense.bias"])
        x = bo.layer_norm(x + ffn, w[f"{p}.output.LayerNorm.weight"], w[f"{p}.output.LayerNorm.bias"])
    for d, n in enumerate(lens):
        if n == 0:
            continue
        acc = x[offsets[d]:offsets[d + 1]].sum(axis=0, dtype=F) * F(1.0 / n)
        norm_sq = F((acc * acc).sum(dtype=F))
        out[d] = acc * F(1.0 / np.sqrt(norm_sq)) if np.isfinite(norm_sq) and norm_sq > F(1.1920929e-7) else 0.0
    return out


def rust_quant_pin_matrix() -> np.ndarray:
    """The fixed [4, 8] matrix of the INTEGRATION.md pin (quantize_per_output_channel_i8 printed by a Rust #[test]).  Row 0 has
    amax 127 (inv = 1 exactly): its entries +-0.5, +-1.5, +-2.5 are exact ties.  Row 1 is all zeros.  Row 2 has amax 2.54
    (x * inv lands next to .5 after f32 rounding).  Row 3 mixes a large and tiny magnitudes."""
    return np.array([
        [127.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999997],
        [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0],
        [2.54, 0.01, -0.01, 0.03, -0.05, 1.27, -2.54, 0.0],
        [-1000.0, 3.9370079, -3.9370079, 11.811024, 0.001, -0.5, 500.0, 250.0],
    ], dtype=F)

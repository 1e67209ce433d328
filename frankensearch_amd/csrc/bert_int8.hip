// bert_int8.hip — the int8 dynamic-quant linears of the MiniLM-class encoder (FSGPU_BERT_LINEAR_INT8_DYNAMIC), the arithmetic
// class of the reference's own native forward: every Linear weight int8 per output channel (quantize_per_output_channel_i8 at load,
// crates/frankensearch-rerank/src/native.rs:1506,1581), every Linear input int8 per row at forward (linear_int8_dynamic_f32,
// native.rs:543-553), i32 accumulation, f32 epilogue.  Embeddings, LayerNorm, softmax, GELU and the residual stream stay f32.
//
// Quantisation contract (the same formula for weight rows and activation rows — both go through i8_row_scale /
// i8_code below):
//   amax = max_k |x[k]|;  inv = 127.0f / amax;  q[k] = clamp(round_half_away(x[k] * inv), -127, 127);  scale = amax / 127.0f
//   an all-zero row gives q = 0 and scale = 0.  Both divisions are IEEE f32 (this file is built without fast-math).
//   a row with 0 < amax < 127 / FLT_MAX has inv = +inf: its zeros code to 0, its other elements to +-127 (NaN and Inf inputs: undefined).
// Epilogue: y = ((float)acc * (sx[m] * sw[n])) + b[n] as separate multiplies and an add (-ffp-contract=off).
//
// GEMM: v_mfma_i32_16x16x64_i8, A = the activation codes [M, K] row-major, B = the weight codes pre-packed in fragment order (a
// 16 x 64 tile is 1 KB: lane l's 16 bytes are row l & 15, k 16 (l >> 4) .. + 15).  The accumulation is exact in i32, so a row's
// result depends on nothing but that row and the weights: whatever M, tile or batch it rides in, it has the same bits.
#include <cstdint>

#include "device_util.hpp"
#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

__device__ __forceinline__ float i8_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float i8_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}

// exact-form GELU with the Abramowitz-Stegun 7.1.26 erf (native.rs:190-200); the same statement as bert_kernels.hip's gelu_as
__device__ __forceinline__ float i8_gelu(float x) {
    const float z = x * 0.70710678118654752440f;
    const float az = fabsf(z);
    const float t = 1.0f / (1.0f + 0.3275911f * az);
    const float poly =
        t * (0.2548296f + t * (-0.28449673f + t * (1.4214137f + t * (-1.453152f + t * 1.0614054f))));
    const float erf_abs = 1.0f - poly * __expf(-(z * z));
    const float erf = copysignf(erf_abs, z);
    return 0.5f * x * (1.0f + erf);
}

// The quantisation contract, shared by the weight packer and every activation quantiser.  amax == 0: inv = 0, every code 0.
// 0 < amax < 127 / FLT_MAX (~ 3.7e-37): inv = +inf; a non-zero element's product is +-inf and its code +-127, a zero element's
// product is NaN and its code 0 (the tiny-amax rule of DESIGN §3.8: a zero codes to 0 in every row).
__device__ __forceinline__ float i8_row_inv(float amax) { return amax > 0.f ? 127.0f / amax : 0.f; }
__device__ __forceinline__ float i8_row_scale(float amax) { return amax / 127.0f; }
__device__ __forceinline__ int8_t i8_code(float v, float inv) {
    const float p = v * inv;
    const float r = roundf(p == p ? p : 0.f);   // half away from zero (Rust f32::round); NaN only as 0 * inf
    return (int8_t)(int)fminf(fmaxf(r, -127.0f), 127.0f);
}

constexpr int kI8MaxPerLane = 16;  // hidden <= 1024

__device__ __forceinline__ float to_f32(float v) { return v; }
__device__ __forceinline__ float to_f32(_Float16 v) { return (float)v; }

// LayerNorm of one row held as v[per] per lane (element lane + 64 i; the statement of bert_kernels.hip's row_layer_norm), the f32
// result to x_out, then (q non-null) the row's int8 codes and scale.
__device__ __forceinline__ void ln_quant_row(float (&v)[kI8MaxPerLane], int per, int hidden, const float* w, const float* b, float eps,
                                             float* x_out, int8_t* q, float* s, int lane) {
    float sum = 0.f;
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) sum += v[i];
    const float mean = i8_wave_sum(sum) / (float)hidden;
    float sq = 0.f;
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) {
            const float d = v[i] - mean;
            sq += d * d;
        }
    const float var = i8_wave_sum(sq) / (float)hidden;
    const float inv_std = 1.0f / sqrtf(var + eps);
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) {
            const int d = lane + 64 * i;
            v[i] = (v[i] - mean) * inv_std * w[d] + b[d];
            x_out[d] = v[i];
            amax = fmaxf(amax, fabsf(v[i]));
        }
    if (!q) return;
    amax = i8_wave_max(amax);
    const float inv = i8_row_inv(amax);
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) q[lane + 64 * i] = i8_code(v[i], inv);
    if (lane == 0) *s = i8_row_scale(amax);
}

}  // namespace

// Stand-alone row quantiser (the attention context, the GELU output): one wave per row, two passes over the row (the second
// from cache).  Any K.
template <typename T>
__global__ __launch_bounds__(256) void bert_i8_quant_rows_kernel(const T* __restrict__ x, int8_t* __restrict__ q,
                                                                 float* __restrict__ s, int rows, int K) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= rows) return;
    const T* xr = x + (size_t)r * K;
    float amax = 0.f;
    for (int k = lane; k < K; k += 64) amax = fmaxf(amax, fabsf(to_f32(xr[k])));
    amax = i8_wave_max(amax);
    const float inv = i8_row_inv(amax);
    int8_t* qr = q + (size_t)r * K;
    for (int k = lane; k < K; k += 64) qr[k] = i8_code(to_f32(xr[k]), inv);
    if (lane == 0) s[r] = i8_row_scale(amax);
}

// Weight packer (load time): row n of W [N, K] f32 -> its scale sw[n] and its codes in fragment order (the tile (n >> 4, k >> 6)
// is 64 lanes x 16 bytes; lane (n & 15) + 16 ((k & 63) >> 4), byte k & 15).  One wave per output channel.
__global__ __launch_bounds__(256) void bert_i8_pack_w_kernel(const float* __restrict__ w, int8_t* __restrict__ wp,
                                                             float* __restrict__ sw, int N, int K) {
    const int lane = threadIdx.x & 63;
    const int n = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (n >= N) return;
    const float* wr = w + (size_t)n * K;
    float amax = 0.f;
    for (int k = lane; k < K; k += 64) amax = fmaxf(amax, fabsf(wr[k]));
    amax = i8_wave_max(amax);
    const float inv = i8_row_inv(amax);
    const int kc = K >> 6;
    for (int k = lane; k < K; k += 64) {
        const size_t tile = (size_t)(n >> 4) * kc + (k >> 6);
        const int l = (n & 15) + 16 * ((k & 63) >> 4);
        wp[(tile * 64 + l) * 16 + (k & 15)] = i8_code(wr[k], inv);
    }
    if (lane == 0) sw[n] = i8_row_scale(amax);
}

// word + position + token_type(0) embedding, LayerNorm, int8 codes of the result.  One wave per token.
__global__ __launch_bounds__(256) void bert_i8_embed_ln_quant_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ positions,
                                                                     const float* __restrict__ word, const float* __restrict__ pos,
                                                                     const float* __restrict__ type0, const float* __restrict__ lnw,
                                                                     const float* __restrict__ lnb, float* __restrict__ x,
                                                                     int8_t* __restrict__ q, float* __restrict__ s, int tokens, int hidden,
                                                                     float eps) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tokens) return;
    const int per = hidden >> 6;
    const float* wr = word + (size_t)ids[t] * hidden;
    const float* pr = pos + (size_t)positions[t] * hidden;
    float v[kI8MaxPerLane];
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) {
            const int d = lane + 64 * i;
            v[i] = (wr[d] + pr[d]) + type0[d];
        }
    ln_quant_row(v, per, hidden, lnw, lnb, eps, x + (size_t)t * hidden, q ? q + (size_t)t * hidden : nullptr, s + t, lane);
}

// x = LayerNorm(x + delta) in place (add_ln_raw, native.rs:560-578), then the int8 codes of the new x (q may be null: the last
// layer's output feeds only the pooling).  One wave per token.
__global__ __launch_bounds__(256) void bert_i8_add_ln_quant_kernel(float* __restrict__ x, const float* __restrict__ delta,
                                                                   const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                                   int8_t* __restrict__ q, float* __restrict__ s, int tokens, int hidden,
                                                                   float eps) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tokens) return;
    const int per = hidden >> 6;
    float* xr = x + (size_t)t * hidden;
    const float* dr = delta + (size_t)t * hidden;
    float v[kI8MaxPerLane];
#pragma unroll
    for (int i = 0; i < kI8MaxPerLane; ++i)
        if (i < per) v[i] = xr[lane + 64 * i] + dr[lane + 64 * i];
    ln_quant_row(v, per, hidden, lnw, lnb, eps, xr, q ? q + (size_t)t * hidden : nullptr, s + t, lane);
}

// out[M, N] = dequant(qa [M, K] x wp^T) + bias (EPI 1: then GELU).  A 256-thread block is 2 x 2 waves over a 64 x 128 output tile; a
// wave owns 32 x 64 (2 x 4 MFMA tiles, 32 accumulator registers) and reads its A fragments (16 bytes of one row per lane) and B
// fragments (1 KB per tile, coalesced) straight from L2.  Rows past M are read clamped and never written.  K % 64 == 0,
// N % 64 == 0 (bert_i8_gemm_supported).
template <int EPI>
__global__ __launch_bounds__(256) void bert_i8_gemm_kernel(const int8_t* __restrict__ qa, const float* __restrict__ sa,
                                                           const i32x4* __restrict__ wp, const float* __restrict__ sw,
                                                           const float* __restrict__ bias, float* __restrict__ out, int M, int N, int K) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int m0 = blockIdx.y * 64 + (wave >> 1) * 32;
    const int n0 = blockIdx.x * 128 + (wave & 1) * 64;
    if (m0 >= M || n0 >= N) return;   // wave-uniform; no block-level synchronisation below
    const int fr = lane & 15, kg = lane >> 4;
    const int kc_n = K >> 6;
    const int8_t* arow[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int r = m0 + i * 16 + fr;
        arow[i] = qa + (size_t)(r < M ? r : M - 1) * K + kg * 16;
    }
    const i32x4* bt[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) bt[j] = wp + (size_t)((n0 >> 4) + j) * kc_n * 64 + lane;
    i32x4 acc[2][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = i32x4{0, 0, 0, 0};
    for (int kc = 0; kc < kc_n; ++kc) {
        i32x4 a[2], b[4];
#pragma unroll
        for (int i = 0; i < 2; ++i) a[i] = *reinterpret_cast<const i32x4*>(arow[i] + kc * 64);
#pragma unroll
        for (int j = 0; j < 4; ++j) b[j] = bt[j][(size_t)kc * 64];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_i32_16x16x64_i8(a[i], b[j], acc[i][j], 0, 0, 0);
    }
    // C layout: column = lane & 15, row = (lane >> 4) * 4 + register
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const int n = n0 + j * 16 + fr;
        const float swn = sw[n], bn = bias[n];
#pragma unroll
        for (int i = 0; i < 2; ++i)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = m0 + i * 16 + kg * 4 + r;
                if (m < M) {
                    const float scale = sa[m] * swn;
                    float y = (float)acc[i][j][r] * scale + bn;
                    if (EPI == 1) y = i8_gelu(y);
                    out[(size_t)m * N + n] = y;
                }
            }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------

// The shape rule alone.  The accumulator is i32 and 127 x 127 x K must stay below 2^31: K <= 133,120.  The encoder's K is at most its
// intermediate width, and the lab entry (fsgpu_lab_bert_int8_stage) caps K at 4096.
bool bert_i8_gemm_supported(int N, int K) { return N > 0 && K > 0 && N % 64 == 0 && K % 64 == 0; }

size_t bert_i8_packed_bytes(int N, int K) { return (size_t)N * K; }

hipError_t launch_bert_i8_pack_w(const float* w, void* wp, float* sw, int N, int K, hipStream_t stream) {
    if (!bert_i8_gemm_supported(N, K)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bert_i8_pack_w_kernel, dim3((N + 3) / 4), dim3(256), 0, stream, w, static_cast<int8_t*>(wp), sw, N, K);
    return hipGetLastError();
}

hipError_t launch_bert_i8_quant_rows(const float* x, void* q, float* s, int rows, int K, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(bert_i8_quant_rows_kernel<float>, dim3((rows + 3) / 4), dim3(256), 0, stream, x, static_cast<int8_t*>(q), s, rows, K);
    return hipGetLastError();
}

hipError_t launch_bert_i8_quant_rows_h(const void* x_h, void* q, float* s, int rows, int K, hipStream_t stream) {
    if (rows <= 0) return hipSuccess;
    hipLaunchKernelGGL(bert_i8_quant_rows_kernel<_Float16>, dim3((rows + 3) / 4), dim3(256), 0, stream, static_cast<const _Float16*>(x_h),
                       static_cast<int8_t*>(q), s, rows, K);
    return hipGetLastError();
}

hipError_t launch_bert_i8_embed_ln_quant(const int32_t* ids, const int32_t* positions, const float* word, const float* pos,
                                         const float* type0, const float* lnw, const float* lnb, float* x, void* q, float* s, int tokens,
                                         int hidden, float eps, hipStream_t stream) {
    if (tokens <= 0) return hipSuccess;
    if (hidden % 64 != 0 || hidden > 64 * kI8MaxPerLane) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bert_i8_embed_ln_quant_kernel, dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, positions, word, pos, type0, lnw,
                       lnb, x, static_cast<int8_t*>(q), s, tokens, hidden, eps);
    return hipGetLastError();
}

hipError_t launch_bert_i8_add_ln_quant(float* x, const float* delta, const float* lnw, const float* lnb, void* q, float* s, int tokens,
                                       int hidden, float eps, hipStream_t stream) {
    if (tokens <= 0) return hipSuccess;
    if (hidden % 64 != 0 || hidden > 64 * kI8MaxPerLane) return hipErrorInvalidValue;
    hipLaunchKernelGGL(bert_i8_add_ln_quant_kernel, dim3((tokens + 3) / 4), dim3(256), 0, stream, x, delta, lnw, lnb,
                       static_cast<int8_t*>(q), s, tokens, hidden, eps);
    return hipGetLastError();
}

hipError_t launch_bert_i8_gemm(const void* qa, const float* sa, const void* wp, const float* sw, const float* bias, float* out, int M,
                               int N, int K, bool gelu, hipStream_t stream) {
    if (!bert_i8_gemm_supported(N, K)) return hipErrorInvalidValue;
    if (M <= 0) return hipSuccess;
    const dim3 grid((N + 127) / 128, (M + 63) / 64);
    const int8_t* a = static_cast<const int8_t*>(qa);
    const i32x4* b = static_cast<const i32x4*>(wp);
    if (gelu) hipLaunchKernelGGL(bert_i8_gemm_kernel<1>, grid, dim3(256), 0, stream, a, sa, b, sw, bias, out, M, N, K);
    else hipLaunchKernelGGL(bert_i8_gemm_kernel<0>, grid, dim3(256), 0, stream, a, sa, b, sw, bias, out, M, N, K);
    return hipGetLastError();
}

}  // namespace fsgpu

// bert_rerank.hip — the cross-encoder kernels of the GPU reranker (bert_reranker.cpp), for gfx950.
//
// The reference's NativeReranker (crates/frankensearch-rerank/src/native.rs:1240) runs a BertForSequenceClassification over
// `[CLS] query [SEP] doc [SEP]` pairs: typed embeddings, the encoder's layers, the last layer for the [CLS] rows only
// (encoder_layer_cls, native.rs:628-700; fused_attention_cls, :438-482), then pooler (dense + tanh) and a 1-logit classifier
// (forward_batch, :956-1130).  Every layer but the last, and the last layer's QKV projection, are the embedder's fragment-order
// kernels (bert_gemm_w.hip, bert_kernels.hip); what is here is the part the embedder lacks:
//   bert_embed_typed_ln_kernel   word[id] + pos[p] + type[type_id], then LayerNorm (f32 and f16 copies, as the layer chain reads them)
//   bert_cls_attention_kernel    the [CLS] query of a pair against all of its keys, per head; also gathers the pair's [CLS] residual row
//   bert_cls_head_kernel         pooled = tanh(W_p cls + b_p), logit = w_c . pooled + b_c, score = sigmoid(logit) (0 if not finite)
// Every kernel computes a pair's (a token's) values from that pair (token) alone, in an order fixed by the model's shape: a pair's
// logit has the same bits whatever call, batch or position it rides in.
#include "device_util.hpp"
#include "kernels.hpp"

namespace fsgpu {

namespace {
__device__ __forceinline__ float rr_wave_sum(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off);
    return v;
}
__device__ __forceinline__ float rr_wave_max(float v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmaxf(v, __shfl_xor(v, off));
    return v;
}
constexpr int kRrMaxPerLane = 16;   // hidden <= 1024
constexpr int kRrMaxSeq = 512;      // a pair's tokens (max_position_embeddings, DEFAULT_MAX_LENGTH native.rs:41-51)
}  // namespace

// One wave per token: v = (word[id] + pos[p]) + type[type_id] (native.rs:1176-1192 with the pair's token types), LayerNorm with the
// statistics in f32, written as f32 (the residual stream) and f16 (the next projection's operand).
__global__ __launch_bounds__(256) void bert_embed_typed_ln_kernel(const int32_t* __restrict__ ids, const int32_t* __restrict__ types,
                                                                  const int32_t* __restrict__ positions, const float* __restrict__ word,
                                                                  const float* __restrict__ pos, const float* __restrict__ type_emb,
                                                                  const float* __restrict__ lnw, const float* __restrict__ lnb,
                                                                  float* __restrict__ x_f32, _Float16* __restrict__ x_h, int tokens,
                                                                  int hidden, float eps) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= tokens) return;
    const int per = hidden >> 6;
    const float* wr = word + (size_t)ids[t] * hidden;
    const float* pr = pos + (size_t)positions[t] * hidden;
    const float* tr = type_emb + (size_t)types[t] * hidden;
    float v[kRrMaxPerLane];
    float s = 0.f;
#pragma unroll
    for (int i = 0; i < kRrMaxPerLane; ++i)
        if (i < per) {
            const int d = lane + 64 * i;
            v[i] = (wr[d] + pr[d]) + tr[d];
            s += v[i];
        }
    const float mean = rr_wave_sum(s) / (float)hidden;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < kRrMaxPerLane; ++i)
        if (i < per) {
            const float d = v[i] - mean;
            q += d * d;
        }
    const float inv = 1.0f / sqrtf(rr_wave_sum(q) / (float)hidden + eps);
    float* xo = x_f32 + (size_t)t * hidden;
    _Float16* ho = x_h + (size_t)t * hidden;
#pragma unroll
    for (int i = 0; i < kRrMaxPerLane; ++i)
        if (i < per) {
            const int d = lane + 64 * i;
            const float y = (v[i] - mean) * inv * lnw[d] + lnb[d];
            xo[d] = y;
            ho[d] = (_Float16)y;
        }
}

// One wave per (pair, head): the pair's first token (its [CLS]) as the only query against all S keys of the pair, over the f16 Q / K / V
// the last layer's QKV projection wrote for every token ([T, 3H]: Q | K | V, head h at columns h*32 .. +32).  Softmax in the
// reference's form, exp((x - max) * scale) / sum (softmax_row_fused, native.rs:82-147): scores are f32 dot products over the 32
// dimensions in order; lane l holds keys l, l + 64, ...; max and sum are butterfly reductions.  ctx_cls [n_pairs, H] f16 (the output
// projection's operand); the block also copies the pair's [CLS] residual row x[t0] (f32) to x_cls — the rows the rest of the last layer
// runs on.
__global__ __launch_bounds__(64) void bert_cls_attention_kernel(const _Float16* __restrict__ qkv, const uint32_t* __restrict__ offsets,
                                                                const float* __restrict__ x, _Float16* __restrict__ ctx_cls,
                                                                float* __restrict__ x_cls, int hidden, float scale) {
    __shared__ float p_s[kRrMaxSeq];
    __shared__ float part[2][32];
    const int pair = blockIdx.x, head = blockIdx.y;
    const int lane = threadIdx.x;
    const uint32_t t0 = offsets[pair];
    const int S = (int)(offsets[pair + 1] - t0);
    const int d = lane & 31;
    if (lane < 32) x_cls[(size_t)pair * hidden + head * 32 + d] = x[(size_t)t0 * hidden + head * 32 + d];
    if (S <= 0 || S > kRrMaxSeq) return;   // (the host never sends an empty or over-long pair)
    const int stride = 3 * hidden;
    const _Float16* base = qkv + (size_t)t0 * stride + head * 32;
    float q[32];
#pragma unroll
    for (int i = 0; i < 32; i += 8) {
        const half8 h = *reinterpret_cast<const half8*>(base + i);
#pragma unroll
        for (int j = 0; j < 8; ++j) q[i + j] = (float)h[j];
    }
    float mx = -INFINITY;
    for (int k = lane; k < S; k += 64) {
        const _Float16* kr = base + (size_t)k * stride + hidden;
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < 32; i += 8) {
            const half8 h = *reinterpret_cast<const half8*>(kr + i);
#pragma unroll
            for (int j = 0; j < 8; ++j) s += q[i + j] * (float)h[j];
        }
        p_s[k] = s;
        mx = fmaxf(mx, s);
    }
    mx = rr_wave_max(mx);
    float sum = 0.f;
    for (int k = lane; k < S; k += 64) {
        const float e = expf((p_s[k] - mx) * scale);
        p_s[k] = e;
        sum += e;
    }
    sum = rr_wave_sum(sum);
    __syncthreads();
    // weighted sum of V: lane (half, d) takes dimension d over the keys of parity half, in key order; the halves meet in LDS
    const int half = lane >> 5;
    float acc = 0.f;
    for (int k = half; k < S; k += 2) acc += p_s[k] * (float)base[(size_t)k * stride + 2 * hidden + d];
    part[half][d] = acc;
    __syncthreads();
    if (lane < 32) {
        const float o = (part[0][d] + part[1][d]) * (1.0f / sum);
        ctx_cls[(size_t)pair * hidden + head * 32 + d] = (_Float16)o;
    }
}

// One 1,024-thread block per pair: pooled[j] = tanh(W_p[j] . cls + b_p[j]) (BertPooler, f32), then logit = w_c . pooled + b_c and
// score = 1 / (1 + exp(-logit)) when the logit is finite, else 0 (rerank_sync, native.rs:1631-1710).  Wave w takes outputs w, w + 16,
// ... four at a time (four weight rows in flight: the loop is latency-bound — one output per iteration with 4 waves measured ~200 us
// per block); a lane sums dims lane + 64 i in order, the wave's butterfly adds the lanes: a fixed order per pair.
__global__ __launch_bounds__(1024) void bert_cls_head_kernel(const float* __restrict__ x_cls, const float* __restrict__ pool_w,
                                                             const float* __restrict__ pool_b, const float* __restrict__ cls_w,
                                                             const float* __restrict__ cls_b, float* __restrict__ logits,
                                                             float* __restrict__ scores, int hidden) {
    constexpr int NW = 16, U = 4;
    __shared__ float cls[1024];
    __shared__ float pooled[1024];
    const int pair = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int per = hidden >> 6;
    for (int i = tid; i < hidden; i += 1024) cls[i] = x_cls[(size_t)pair * hidden + i];
    __syncthreads();
    float c[kRrMaxPerLane];
#pragma unroll
    for (int i = 0; i < kRrMaxPerLane; ++i) c[i] = i < per ? cls[lane + 64 * i] : 0.f;
    for (int j0 = wave * U; j0 < hidden; j0 += NW * U) {
        float s[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int j = j0 + u < hidden ? j0 + u : hidden - 1;
            const float* wr = pool_w + (size_t)j * hidden;
            s[u] = 0.f;
#pragma unroll
            for (int i = 0; i < kRrMaxPerLane; ++i)
                if (i < per) s[u] += wr[lane + 64 * i] * c[i];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const float v = rr_wave_sum(s[u]);
            if (lane == 0 && j0 + u < hidden) pooled[j0 + u] = tanhf(v + pool_b[j0 + u]);
        }
    }
    __syncthreads();
    if (wave == 0) {
        float s = 0.f;
#pragma unroll
        for (int i = 0; i < kRrMaxPerLane; ++i)
            if (i < per) s += cls_w[lane + 64 * i] * pooled[lane + 64 * i];
        s = rr_wave_sum(s);
        if (lane == 0) {
            const float logit = s + cls_b[0];
            logits[pair] = logit;
            scores[pair] = __builtin_isfinite(logit) ? 1.0f / (1.0f + expf(-logit)) : 0.0f;
        }
    }
}

// ---- launchers ------------------------------------------------------------------------------------------

bool bert_rerank_supported(int hidden) { return hidden > 0 && hidden % 64 == 0 && hidden <= 1024; }

hipError_t launch_bert_embed_typed_ln(const int32_t* ids, const int32_t* types, const int32_t* positions, const float* word,
                                      const float* pos, const float* type_emb, const float* lnw, const float* lnb, float* x_f32,
                                      void* x_h, int tokens, int hidden, float eps, hipStream_t stream) {
    if (!bert_rerank_supported(hidden) || tokens < 0) return hipErrorInvalidValue;
    if (tokens == 0) return hipSuccess;
    hipLaunchKernelGGL(bert_embed_typed_ln_kernel, dim3((tokens + 3) / 4), dim3(256), 0, stream, ids, types, positions, word, pos,
                       type_emb, lnw, lnb, x_f32, static_cast<_Float16*>(x_h), tokens, hidden, eps);
    return hipGetLastError();
}

hipError_t launch_bert_cls_attention(const void* qkv_h, const uint32_t* offsets, const float* x, void* ctx_cls_h, float* x_cls,
                                     int n_pairs, int heads, int hidden, float scale, hipStream_t stream) {
    if (!bert_rerank_supported(hidden) || heads * 32 != hidden || n_pairs < 0) return hipErrorInvalidValue;
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(bert_cls_attention_kernel, dim3(n_pairs, heads), dim3(64), 0, stream, static_cast<const _Float16*>(qkv_h),
                       offsets, x, static_cast<_Float16*>(ctx_cls_h), x_cls, hidden, scale);
    return hipGetLastError();
}

hipError_t launch_bert_cls_head(const float* x_cls, const float* pool_w, const float* pool_b, const float* cls_w, const float* cls_b,
                                float* logits, float* scores, int n_pairs, int hidden, hipStream_t stream) {
    if (!bert_rerank_supported(hidden) || n_pairs < 0) return hipErrorInvalidValue;
    if (n_pairs == 0) return hipSuccess;
    hipLaunchKernelGGL(bert_cls_head_kernel, dim3(n_pairs), dim3(1024), 0, stream, x_cls, pool_w, pool_b, cls_w, cls_b, logits, scores,
                       hidden);
    return hipGetLastError();
}

}  // namespace fsgpu

// hash_embed_kernels.hip — HashEmbedder: tokenize -> FNV-1a -> modular / JL projection -> L2, from raw text bytes (gfx950).
//
// Replaces HashEmbedder::embed_sync for a batch of texts (crates/frankensearch-embed/src/hash_embedder.rs):
//   tokenize               :601-685   == text.split(|c| !c.is_alphanumeric()).filter(|t| t.len() >= 2) (:691-695), len in UTF-8 bytes
//   fnv1a_hash             :588-595   offset 0xcbf29ce484222325, prime 0x100000001b3; per byte xor, then wrapping multiply
//   embed_fnv_modular      :263-280   bucket = hash % dimension, +1 when hash >> 63 == 1, else -1
//   embed_jl               :299-346   state = (seed ^ hash) | 1; per dimension three xorshift steps BEFORE the read, +1 when even
//   l2_normalize_in_place  crates/frankensearch-core/src/traits.rs:606-618
// Bit-exact by construction: the accumulator only ever holds exact small integers (|value| <= tokens < 2^24, :294-298), so token
// order, lane grouping and the popcount form (:348-356) cannot change a bit; it is kept as int32 and converted once.  The squared
// norm is then folded left to right by one lane with separate multiply and add, and the scale is 1 / sqrt, both correctly rounded.
//
// One workgroup of four waves per text.  Lanes stride over the bytes; the lane whose byte starts a token walks the token to its
// end (bounded by the text's end) hashing as it goes.  FNV: one LDS integer atomic per token.  JL: the kept states are compacted
// (ballot / mbcnt) into an LDS list; a wave takes 64 of them, one chain per lane, and per dimension one __ballot and one popcount
// give the sum of the 64 signs, which lane d & 63 adds to its accumulator d >> 6 (16 registers for dim <= 1,024, static index).
// Which characters above U+007F are alphanumeric is the caller's table (one bit per code point); without one the host refuses
// such texts before anything is launched.
#pragma clang fp contract(off)

#include "hash_embedder.hpp"

namespace fsgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kBlocks = (int)(kHashEmbedMaxDim / 64);   // accumulators of a JL lane
constexpr uint32_t kChunk = kHashEmbedChunkStates;     // LDS state list; flushed while a stride of bytes still fits
constexpr u64 kFnvOffset = 0xcbf29ce484222325ull;
constexpr u64 kFnvPrime = 0x100000001b3ull;

// The character that begins at t[p] (p < end): its byte length (clipped to the text) and whether it is alphanumeric.
// Reads nothing at or past `end`; a sequence cut short by the text's end, a stray continuation byte and a value past
// U+10FFFF are non-alphanumeric one-unit characters (the host has refused such texts: this only keeps every read in bounds).
__device__ __forceinline__ bool char_at(const uint8_t* __restrict__ t, uint32_t p, uint32_t end, const uint8_t* __restrict__ bitmap,
                                        uint32_t& len) {
    const uint32_t b0 = t[p];
    if (b0 < 0x80u) {
        len = 1;
        return (b0 - '0') < 10u || ((b0 | 0x20u) - 'a') < 26u;   // u8::is_ascii_alphanumeric
    }
    uint32_t need = b0 >= 0xf0u ? 4u : b0 >= 0xe0u ? 3u : b0 >= 0xc0u ? 2u : 1u;
    if (need == 1u || need > end - p) {
        len = 1;
        return false;
    }
    uint32_t cp = b0 & (0xffu >> (need + 1u));
    for (uint32_t i = 1; i < need; ++i) cp = (cp << 6) | (t[p + i] & 0x3fu);
    len = need;
    if (!bitmap || cp >= kHashEmbedCodePoints) return false;
    return (bitmap[cp >> 3] >> (cp & 7u)) & 1u;
}

// Does a token start at byte p of the text [begin, end)?  Its character is alphanumeric and it is the text's first byte or
// follows a non-alphanumeric character (the previous character begins at most 3 continuation bytes back, never before begin).
__device__ __forceinline__ bool token_starts(const uint8_t* __restrict__ t, uint32_t p, uint32_t begin, uint32_t end,
                                             const uint8_t* __restrict__ bitmap) {
    if ((t[p] & 0xc0u) == 0x80u) return false;   // inside a character
    uint32_t len;
    if (!char_at(t, p, end, bitmap, len)) return false;
    if (p == begin) return true;
    uint32_t q = p - 1;
    for (int back = 0; back < 3 && q > begin && (t[q] & 0xc0u) == 0x80u; ++back) --q;
    return !char_at(t, q, p, bitmap, len);
}

// hash % dim without a 64-bit division: hash = hi * 2^32 + lo, every product below 2^20 for dim <= 1,024.
__device__ __forceinline__ uint32_t bucket_of(u64 hash, uint32_t dim) {
    const uint32_t hi = (uint32_t)(hash >> 32), lo = (uint32_t)hash;
    const uint32_t two32 = (0xffffffffu % dim + 1u) % dim;
    return ((hi % dim) * two32 + lo % dim) % dim;
}

template <bool JL>
__global__ __launch_bounds__(kThreads) void hash_embed_kernel(HashEmbedArgs a) {
    __shared__ int acc[kHashEmbedMaxDim];     // the accumulator, exact integers
    __shared__ float vec[kHashEmbedMaxDim];   // ... as f32, for the sequential fold
    __shared__ u64 states[JL ? kChunk : 1];
    __shared__ uint32_t s_fill, s_tokens;
    __shared__ float s_scale;

    const uint32_t text = blockIdx.x;
    const uint32_t begin = a.offsets[text], end = a.offsets[text + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t dim = a.dim;
    const uint8_t* __restrict__ t = a.text;

    for (uint32_t d = tid; d < dim; d += kThreads) acc[d] = 0;
    if (tid == 0) {
        s_fill = 0;
        s_tokens = 0;
    }
    __syncthreads();

    int part[kBlocks];   // JL: this lane's share of the accumulator (dimension b * 64 + lane)
#pragma unroll
    for (int b = 0; b < kBlocks; ++b) part[b] = 0;
    uint32_t my_tokens = 0;   // FNV: tokens this lane hashed

    for (uint32_t base = begin;; base += kThreads) {   // (end - begin <= 32 MiB: base + kThreads cannot wrap)
        const uint32_t p = base + tid;
        bool keep = false;
        u64 h = kFnvOffset;
        if (p < end && token_starts(t, p, begin, end, a.bitmap)) {
            uint32_t q = p;
            while (q < end) {   // the token: bounded by the text's end
                uint32_t len;
                if (!char_at(t, q, end, a.bitmap, len)) break;
                for (uint32_t i = 0; i < len; ++i) h = (h ^ (u64)t[q + i]) * kFnvPrime;
                q += len;
            }
            keep = q - p >= 2u;   // MIN_TOKEN_LEN, in bytes
        }
        const bool last = end - base <= (uint32_t)kThreads;   // (base <= end throughout)
        if (!JL) {
            if (keep) {
                atomicAdd(&acc[bucket_of(h, dim)], (h >> 63) == 1ull ? 1 : -1);
                ++my_tokens;
            }
            if (last) break;
            continue;
        }
        // ---- JL: compact the kept states into the LDS list (order is free: the sums are exact) ----
        const u64 m = __ballot(keep);
        if (m != 0ull) {
            uint32_t at = 0;
            if (lane == 0) at = atomicAdd(&s_fill, (uint32_t)__popcll(m));
            at = __shfl(at, 0);
            if (keep) states[at + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = (a.seed ^ h) | 1ull;
        }
        __syncthreads();
        const uint32_t fill = s_fill;   // <= kChunk: a flush leaves room for one more stride of kThreads states
        __syncthreads();                // every wave has read it (and decides alike) before a wave of the next stride adds to it
        if (last || fill > kChunk - kThreads) {
            if (tid == 0) {             // (the next stride's appends come after the barrier below)
                s_tokens += fill;
                s_fill = 0;
            }
            for (uint32_t g = wave * 64u; g < fill; g += kWaves * 64u) {   // waves take alternate groups of 64 chains
                const bool live = g + lane < fill;
                u64 s = live ? states[g + lane] : 1ull;
                const u64 active = __ballot(live);
                const int n_active = (int)__popcll(active);
#pragma unroll
                for (int b = 0; b < kBlocks; ++b) {
                    if ((uint32_t)b * 64u >= dim) break;   // uniform
                    const uint32_t width = dim - (uint32_t)b * 64u < 64u ? dim - (uint32_t)b * 64u : 64u;
                    for (uint32_t j = 0; j < width; ++j) {
                        s ^= s << 13;
                        s ^= s >> 7;
                        s ^= s << 17;
                        const u64 odd = __ballot((s & 1ull) != 0ull) & active;
                        const int sum = n_active - 2 * (int)__popcll(odd);   // (+1 per even chain, -1 per odd one)
                        part[b] += lane == j ? sum : 0;
                    }
                }
            }
            __syncthreads();   // every wave has read its groups: the list may be refilled
        }
        if (last) break;
    }

    if (JL) {
#pragma unroll
        for (int b = 0; b < kBlocks; ++b) {
            const uint32_t d = (uint32_t)b * 64u + lane;
            if (d < dim && part[b] != 0) atomicAdd(&acc[d], part[b]);   // integer: order-free
        }
    } else {
        if (my_tokens != 0u) atomicAdd(&s_tokens, my_tokens);
    }
    __syncthreads();

    // ---- l2_normalize_in_place (traits.rs:606-618): sequential fold, zeros below f32::EPSILON ----
    for (uint32_t d = tid; d < dim; d += kThreads) vec[d] = (float)acc[d];
    __syncthreads();
    if (tid == 0) {
        float norm_sq = 0.f;
        for (uint32_t d = 0; d < dim; ++d) {
            const float sq = vec[d] * vec[d];
            norm_sq = norm_sq + sq;
        }
        float scale = 0.f;
        if (__builtin_isfinite(norm_sq) && !(norm_sq < 1.1920929e-7f)) scale = 1.0f / __builtin_sqrtf(norm_sq);
        s_scale = scale;
        if (a.token_counts) a.token_counts[text] = s_tokens;
    }
    __syncthreads();
    const float scale = s_scale;
    float* __restrict__ o = a.out + (size_t)text * dim;
    for (uint32_t d = tid; d < dim; d += kThreads) o[d] = scale != 0.f ? vec[d] * scale : 0.f;
}

}  // namespace

hipError_t launch_hash_embed(const HashEmbedArgs& args, uint32_t n, bool jl, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    if (args.dim == 0 || args.dim > kHashEmbedMaxDim) return hipErrorInvalidValue;
    if (jl)
        hipLaunchKernelGGL(hash_embed_kernel<true>, dim3(n), dim3(kThreads), 0, stream, args);
    else
        hipLaunchKernelGGL(hash_embed_kernel<false>, dim3(n), dim3(kThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace fsgpu

// mmr_kernels.hip — Maximum Marginal Relevance over rows of the slab, for gfx950 (vector_index_mmr.cpp launches it).
//
// The reference's mmr_rerank (crates/frankensearch-fusion/src/mmr.rs:103-319) on vectors that stay where they are: ONE workgroup
// per pool (grid = number of pools), so a pool's answer is computed from that pool alone, the same for one pool and for 1,024.
//   1. gather    the pool's n rows (f16 or f32 slab rows, or a per-candidate f32 override vector: a WAL entry) into a staging
//                area with padded rows: LDS when it fits, a global workspace for the large f32 pools (a wave per row)
//   2. norms     one lane per candidate: ONE f64 accumulator over the elements in order, then sqrt (mmr.rs:163-175)
//   3. dots      one lane per pair i <= j (sim is bit-symmetric): cosine_sim_pre's FOUR f64 accumulators, element e to acc[e % 4]
//                in ascending order, ((a0 + a1) + a2) + a3, then the tail in order (mmr.rs:285-319); the four chains are
//                independent, which is what keeps the lane's f64 pipe busy
//   4. normalise dot / (root_i * root_j), 0 below f64::EPSILON; both halves of the n x n matrix (LDS, or global when the caller
//                wants the matrix or it does not fit)
//   5. greedy    wave 0 alone, no workgroup barrier inside the loop: min-max normalised relevance, first pick, then k - 1 rounds of
//                fma(lambda, norm_score, -((1 - lambda) * max_sim)) with a wave arg-max (greatest value, lowest index on a tie: what
//                the reference's strict `>` over ascending indexes selects)
// Every product here is exact in f64 (f16 x f16 has at most 22 significant bits, f32 x f32 at most 48), so fma(x, y, acc) and a
// separate multiply and add give the same bits: only the ORDER of the additions is part of the contract, and it is the reference's.
// sqrt and / are the compiler's IEEE expansions (-fno-fast-math); f64 denormals are kept.
#include "device_util.hpp"
#include "kernels.hpp"

namespace fsgpu {

namespace {
constexpr uint32_t kMmrNone = 0xffffffffu;
constexpr double kMmrEpsilon = 2.220446049250313e-16;   // f64::EPSILON

__device__ __forceinline__ void mmr_load4(const _Float16* p, double* v) {
    const uint2 raw = *reinterpret_cast<const uint2*>(p);
    const _Float16* h = reinterpret_cast<const _Float16*>(&raw);
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = (double)(float)h[i];
}
__device__ __forceinline__ void mmr_load4(const float* p, double* v) {
    const float4 raw = *reinterpret_cast<const float4*>(p);
    v[0] = (double)raw.x, v[1] = (double)raw.y, v[2] = (double)raw.z, v[3] = (double)raw.w;
}

// pair p of the lower triangle, column by column: p = j (j + 1) / 2 + i with i <= j (consecutive lanes share row j)
__device__ __forceinline__ void mmr_pair(uint32_t p, uint32_t* i, uint32_t* j) {
    uint32_t c = (uint32_t)((sqrtf(8.0f * (float)p + 1.0f) - 1.0f) * 0.5f);
    while ((c + 1) * (c + 2) / 2 <= p) ++c;
    while (c * (c + 1) / 2 > p) --c;
    *j = c;
    *i = p - c * (c + 1) / 2;
}

struct MmrBest {
    double v;
    uint32_t i;   // kMmrNone: no candidate
};
// the reference scans ascending indexes with a strict `>` from -inf: the greatest value wins, the lowest index among equals
__device__ __forceinline__ MmrBest mmr_better(MmrBest a, MmrBest b) {
    if (b.i == kMmrNone) return a;
    if (a.i == kMmrNone) return b;
    if (a.v > b.v) return a;
    if (b.v > a.v) return b;
    return a.i < b.i ? a : b;
}
__device__ __forceinline__ MmrBest mmr_wave_best(MmrBest x) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        MmrBest y;
        y.v = __shfl_xor(x.v, off);
        y.i = __shfl_xor(x.i, off);
        x = mmr_better(x, y);
    }
    return x;
}
__device__ __forceinline__ MmrBest mmr_candidate(double v, uint32_t i, bool live) {
    MmrBest b;
    b.v = v;
    b.i = (live && v > -INFINITY) ? i : kMmrNone;   // a NaN never beats -inf
    return b;
}
}  // namespace

// T: the staged element type (f16 only for f16 slabs without overrides); kLds: the staged rows live in LDS
template <typename T, bool kLds>
__global__ __launch_bounds__(256) void mmr_kernel(MmrArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mmr_smem[];
    const uint32_t pool = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t begin = a.offsets[pool], len = a.offsets[pool + 1] - begin;
    const uint32_t n = len < a.candidate_pool ? len : a.candidate_pool;
    const uint32_t k = a.k < n ? a.k : n;
    if (n == 0 || k == 0) {
        if (tid == 0) a.out_counts[pool] = 0;
        return;
    }
    if (!mmr_device_pool(n, a.dim)) return;   // the host restatement answers this pool (vector_index_mmr.cpp)
    const uint32_t dim = a.dim, S = a.vec_stride;
    double* norms = reinterpret_cast<double*>(mmr_smem);   // [kMmrMaxPool]
    T* vec;
    if constexpr (kLds) vec = reinterpret_cast<T*>(mmr_smem + kMmrLdsHeader);
    else vec = reinterpret_cast<T*>(a.vec_ws) + (size_t)begin * S;
    double* sims = a.sims ? a.sims + (u64)begin * a.sim_pitch : reinterpret_cast<double*>(mmr_smem + a.lds_sims_offset);

    // 1. gather: a wave per row
    for (uint32_t c = wave; c < n; c += 4) {
        T* dst = vec + (size_t)c * S;
        const int32_t ov = a.ovr_index ? a.ovr_index[begin + c] : -1;
        if (ov >= 0) {
            const float* src = a.ovr_vectors + (size_t)ov * dim;
            for (uint32_t e = lane; e < dim; e += 64) dst[e] = (T)src[e];
        } else {
            const unsigned char* src = static_cast<const unsigned char*>(a.slab) + (size_t)(a.rows[begin + c] - a.row_base) * a.row_stride;
            if (a.slab_f32) {
                const float* s = reinterpret_cast<const float*>(src);
                if constexpr (sizeof(T) == 4) {
                    if ((dim & 3) == 0 && (a.row_stride & 15) == 0) {
                        for (uint32_t e = lane * 4; e < dim; e += 256) *reinterpret_cast<float4*>(dst + e) = *reinterpret_cast<const float4*>(s + e);
                        continue;
                    }
                }
                for (uint32_t e = lane; e < dim; e += 64) dst[e] = (T)s[e];
            } else {
                const _Float16* s = reinterpret_cast<const _Float16*>(src);
                if constexpr (sizeof(T) == 2) {
                    if ((dim & 3) == 0 && (a.row_stride & 7) == 0) {
                        for (uint32_t e = lane * 4; e < dim; e += 256) *reinterpret_cast<uint2*>(dst + e) = *reinterpret_cast<const uint2*>(s + e);
                        continue;
                    }
                }
                for (uint32_t e = lane; e < dim; e += 64) dst[e] = (T)s[e];   // f16 -> f32 is exact
            }
        }
    }
    __syncthreads();

    // 2. root norms: candidate c on lane c / 4 of wave c % 4 (every wave carries the same share of these dim-long chains)
    const uint32_t chunks = dim / 4;
    {
        const uint32_t c = lane * 4 + wave;
        if (c < n) {
            const T* x = vec + (size_t)c * S;
            double s = 0.0, v[4];
#pragma unroll 4   // (the loads of four chunks in flight: the chain itself is dependent)
            for (uint32_t q = 0; q < chunks; ++q) {
                mmr_load4(x + q * 4, v);
                s = fma(v[0], v[0], s);
                s = fma(v[1], v[1], s);
                s = fma(v[2], v[2], s);
                s = fma(v[3], v[3], s);
            }
            for (uint32_t e = chunks * 4; e < dim; ++e) {
                const double xe = (double)(float)x[e];
                s = fma(xe, xe, s);
            }
            norms[c] = sqrt(s);
        }
    }
    // 3. raw dots of the pairs i <= j
    const uint32_t npairs = n * (n + 1) / 2;
    for (uint32_t p = tid; p < npairs; p += 256) {
        uint32_t i, j;
        mmr_pair(p, &i, &j);
        const T* x = vec + (size_t)i * S;
        const T* y = vec + (size_t)j * S;
        double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, xv[4], yv[4];
#pragma unroll 4
        for (uint32_t q = 0; q < chunks; ++q) {
            mmr_load4(x + q * 4, xv);
            mmr_load4(y + q * 4, yv);
            a0 = fma(xv[0], yv[0], a0);
            a1 = fma(xv[1], yv[1], a1);
            a2 = fma(xv[2], yv[2], a2);
            a3 = fma(xv[3], yv[3], a3);
        }
        double dot = ((a0 + a1) + a2) + a3;
        for (uint32_t e = chunks * 4; e < dim; ++e) dot = fma((double)(float)x[e], (double)(float)y[e], dot);
        sims[(size_t)i * n + j] = dot;
    }
    __syncthreads();
    // 4. cosine: every lane finishes the pairs it computed
    for (uint32_t p = tid; p < npairs; p += 256) {
        uint32_t i, j;
        mmr_pair(p, &i, &j);
        const double denom = norms[i] * norms[j];
        const double s = denom < kMmrEpsilon ? 0.0 : sims[(size_t)i * n + j] / denom;
        sims[(size_t)i * n + j] = s;
        sims[(size_t)j * n + i] = s;
    }
    __syncthreads();
    if (wave != 0) return;

    // 5. greedy selection in one wave: lane l owns candidates l and l + 64
    const uint32_t c0 = lane, c1 = lane + 64;
    bool r0 = c0 < n, r1 = c1 < n;
    const double s0 = r0 ? a.scores[begin + c0] : NAN, s1 = r1 ? a.scores[begin + c1] : NAN;
    const bool f0 = r0 && isfinite(s0), f1 = r1 && isfinite(s1);
    double mn = INFINITY, mx = -INFINITY;
    if (f0) mn = s0, mx = s0;
    if (f1) mn = s1 < mn ? s1 : mn, mx = s1 > mx ? s1 : mx;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double on = __shfl_xor(mn, off), ox = __shfl_xor(mx, off);
        mn = on < mn ? on : mn;
        mx = ox > mx ? ox : mx;
    }
    const double range = mx - mn;
    const double ns0 = !f0 ? 0.0 : range < kMmrEpsilon ? 1.0 : (s0 - mn) / range;
    const double ns1 = !f1 ? 0.0 : range < kMmrEpsilon ? 1.0 : (s1 - mn) / range;
    const double lambda = a.lambda, diversity = 1.0 - lambda;
    uint32_t* order = a.out_order + begin;

    MmrBest best = mmr_wave_best(mmr_better(mmr_candidate(ns0, c0, r0), mmr_candidate(ns1, c1, r1)));
    uint32_t pick = best.i == kMmrNone ? 0u : best.i;   // no score above -inf: the fold's initial index
    if (lane == 0) order[0] = pick;
    if (pick == c0) r0 = false;
    if (pick == c1) r1 = false;
    double m0 = r0 ? sims[(size_t)c0 * n + pick] : -INFINITY, m1 = r1 ? sims[(size_t)c1 * n + pick] : -INFINITY;
    uint32_t count = 1;
    for (uint32_t round = 1; round < k; ++round) {
        const double v0 = fma(lambda, ns0, -(diversity * m0)), v1 = fma(lambda, ns1, -(diversity * m1));
        best = mmr_wave_best(mmr_better(mmr_candidate(v0, c0, r0), mmr_candidate(v1, c1, r1)));
        if (best.i == kMmrNone) break;   // wave-uniform
        pick = best.i;
        if (lane == 0) order[count] = pick;
        ++count;
        if (pick == c0) r0 = false;
        if (pick == c1) r1 = false;
        if (r0) {
            const double s = sims[(size_t)c0 * n + pick];
            if (s > m0) m0 = s;
        }
        if (r1) {
            const double s = sims[(size_t)c1 * n + pick];
            if (s > m1) m1 = s;
        }
    }
    if (lane == 0) a.out_counts[pool] = count;
}

MmrPlan mmr_plan(uint32_t max_n, uint32_t dim, bool f32_staging, bool want_sims) {
    MmrPlan p;
    p.vec_stride = ((dim + 3) & ~3u) + 4;   // rows start 8 (f16) / 16 (f32) bytes further along the banks than their neighbour
    const size_t vec_bytes = ((size_t)max_n * p.vec_stride * (f32_staging ? 4 : 2) + 15) & ~(size_t)15;
    const size_t sim_bytes = (size_t)max_n * max_n * 8;
    p.storage = !f32_staging ? kMmrStageLdsF16 : kMmrLdsHeader + vec_bytes <= kMmrLdsBudget ? kMmrStageLdsF32 : kMmrStageGlobalF32;
    size_t lds = kMmrLdsHeader + (p.storage == kMmrStageGlobalF32 ? 0 : vec_bytes);
    p.lds_sims_offset = (uint32_t)lds;
    p.sims_global = want_sims || lds + sim_bytes > kMmrLdsBudget;
    if (!p.sims_global) lds += sim_bytes;
    p.lds_bytes = (uint32_t)lds;
    return p;
}

hipError_t launch_mmr(const MmrArgs& args, uint32_t npools, const MmrPlan& plan, hipStream_t stream) {
    if (npools == 0) return hipSuccess;
    if (plan.lds_bytes > kMmrLdsBudget) return hipErrorInvalidValue;
    auto kern = plan.storage == kMmrStageLdsF16 ? mmr_kernel<_Float16, true>
                : plan.storage == kMmrStageLdsF32 ? mmr_kernel<float, true>
                                                   : mmr_kernel<float, false>;
    if (plan.lds_bytes > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kMmrLdsBudget);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(npools), dim3(256), plan.lds_bytes, stream, args);
    return hipGetLastError();
}

}  // namespace fsgpu

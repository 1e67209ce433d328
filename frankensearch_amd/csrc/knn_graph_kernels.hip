// knn_graph_kernels.hip — the two ends of one step of the k-NN graph build (include/fsgpu.h, fsgpu_index_build_knn_graph).
//
// The graph is DEFINED by the index's own row-level search: knn(i, m) is the top-(m + 1) of the query "row i widened to f32" with
// the entry of row i taken out (or, when more than m lower-numbered duplicates keep row i out of its own list, the last entry
// dropped).  So the build scans nothing itself.  A step is
//   knn_stage_rows_kernel   up to kKnnChunk live source rows of the slab -> an [n, dim] f32 query block (+ their global row ids)
//   the batched search      unchanged (vector_index_batched.cpp): int8 filter, finish in the reference's order, fallbacks
//   knn_emit_kernel         the [n, m + 1] hits -> [n, m] rows (+ sims): self found with a ballot, the tail shifted up, padding
// Both kernels move a few hundred KB per step beside a search that streams the whole slab: contiguous 16-byte accesses where the
// shape allows them and nothing more.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef uint32_t ku32x4 __attribute__((ext_vector_type(4)));
typedef float kf32x4 __attribute__((ext_vector_type(4)));
typedef _Float16 kf16x8 __attribute__((ext_vector_type(8)));

// One wave per source row.  VEC: the row starts on a 16-byte boundary and holds whole 16-byte units (the host checks base, stride and
// dim): a lane loads 16 bytes and stores 16 (f32 slab) or 2 x 16 (f16 slab, widened: exact) — the wave covers the row contiguously.
template <bool F32, bool VEC>
__global__ __launch_bounds__(256) void knn_stage_rows_kernel(KnnStageArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (i >= a.n) return;
    const uint32_t row = a.src_local[i];
    if (lane == 0) a.src_out[i] = a.row_base + row;
    const unsigned char* src = static_cast<const unsigned char*>(a.slab) + (uint64_t)row * a.row_stride;
    float* dst = a.queries + (uint64_t)i * a.dim;
    if constexpr (VEC) {
        if constexpr (F32) {
            const kf32x4* s = reinterpret_cast<const kf32x4*>(src);
            kf32x4* d = reinterpret_cast<kf32x4*>(dst);
            for (uint32_t c = lane; c < a.dim / 4u; c += 64u) d[c] = s[c];
        } else {
            const kf16x8* s = reinterpret_cast<const kf16x8*>(src);
            kf32x4* d = reinterpret_cast<kf32x4*>(dst);
            for (uint32_t c = lane; c < a.dim / 8u; c += 64u) {
                const kf16x8 h = s[c];
                kf32x4 lo, hi;
                lo.x = (float)h[0], lo.y = (float)h[1], lo.z = (float)h[2], lo.w = (float)h[3];
                hi.x = (float)h[4], hi.y = (float)h[5], hi.z = (float)h[6], hi.w = (float)h[7];
                d[2u * c] = lo;
                d[2u * c + 1u] = hi;
            }
        }
    } else {
        for (uint32_t c = lane; c < a.dim; c += 64u) {
            if constexpr (F32) dst[c] = reinterpret_cast<const float*>(src)[c];
            else dst[c] = (float)reinterpret_cast<const _Float16*>(src)[c];
        }
    }
}

// One wave per source, four sources per block.  Lane l holds hit l of the source's m + 1 (beyond its count: padding).  The ballot
// finds the self entry at position p (absent: p = m, which drops the LAST entry); output slot l takes hit l below p and hit l + 1
// from p on.
__global__ __launch_bounds__(256) void knn_emit_kernel(KnnEmitArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= a.n) return;
    const uint32_t k = a.m + 1u;
    uint32_t cnt = a.hit_counts[s];
    if (cnt > k) cnt = k;
    const uint32_t self = a.src[s];
    uint32_t row = kKnnPadRow;
    float sim = 0.0f;
    if (lane < cnt) {
        row = a.hit_rows[(uint64_t)s * k + lane];
        sim = a.hit_scores[(uint64_t)s * k + lane];
    }
    const unsigned long long found = __ballot(lane < cnt && row == self);
    const uint32_t p = found ? (uint32_t)(__ffsll(found) - 1) : a.m;
    const uint32_t from = lane < p ? lane : lane + 1u;   // (lane 63 may ask for 64: its value is not used, m <= 63)
    const uint32_t r = (uint32_t)__shfl((int)row, (int)(from & 63u));
    const float v = __shfl(sim, (int)(from & 63u));
    if (lane < a.m) {
        const bool have = from < cnt;
        a.out_rows[(uint64_t)s * a.m + lane] = have ? r : kKnnPadRow;
        if (a.out_sims) a.out_sims[(uint64_t)s * a.m + lane] = have ? v : 0.0f;
    }
}

}  // namespace

hipError_t launch_knn_stage_rows(const KnnStageArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    const uint32_t unit = a.slab_f32 ? 4u : 8u;   // elements in 16 bytes
    const bool vec = a.dim % unit == 0 && a.row_stride % 16u == 0 && (reinterpret_cast<uintptr_t>(a.slab) & 15u) == 0 &&
                     (reinterpret_cast<uintptr_t>(a.queries) & 15u) == 0;
    const dim3 grid((a.n + 3u) / 4u), block(256);
    if (a.slab_f32) {
        if (vec) hipLaunchKernelGGL((knn_stage_rows_kernel<true, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((knn_stage_rows_kernel<true, false>), grid, block, 0, stream, a);
    } else {
        if (vec) hipLaunchKernelGGL((knn_stage_rows_kernel<false, true>), grid, block, 0, stream, a);
        else hipLaunchKernelGGL((knn_stage_rows_kernel<false, false>), grid, block, 0, stream, a);
    }
    return hipGetLastError();
}

hipError_t launch_knn_emit(const KnnEmitArgs& a, hipStream_t stream) {
    if (a.n == 0 || a.m == 0 || a.m > kKnnMaxM) return a.n == 0 ? hipSuccess : hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_emit_kernel, dim3((a.n + 3u) / 4u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu

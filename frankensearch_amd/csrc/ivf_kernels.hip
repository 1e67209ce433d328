// ivf_kernels.hip — the inverted-file index (include/fsgpu.h, "IVF index"; ivf_index.cpp).
//
//   ivf_assign_kernel         every gated row takes its best centroid: the transposed exact join (join_tile.hpp), the hot path
//   ivf_count_changed_kernel  rows whose list changed between two assignments
//   ivf_list_keys_kernel      assign -> sort keys;  ivf_list_emit_kernel: sorted keys -> offsets and rows
//   ivf_update_kernel         the f64 sequential mean of a list's members, normalised
//   ivf_merge_kernel          a query's best k over the lists of its probed slots
//
// THE ASSIGNMENT'S SCORE.  Row x against centroid c is dot_product_f16_bytes_f32(row bytes, c) (simd.rs:361-446: leftover chunks
// before the tree) in the index's hreduce order — the bits fsgpu_gather_dot(idx, c, [x]) returns.  The order of a dot's additions
// depends on the element index alone, so the rows sit in LDS widened to f32 (exact) and the centroids stream past them on
// join_tile.hpp's tile; the mapping of lanes to the dot's chains is described there.  A row's running list has ONE slot, in lane 0
// of its group: the key (score_ord << 32 | ~centroid), greater is better — score descending under f32::total_cmp with NaN as -inf,
// the lower centroid first.  A row whose every score is NaN therefore goes to list 0.  A row is owned by one group: no atomics.
#pragma clang fp contract(off)

#include "join_tile.hpp"

namespace fsgpu {

namespace {

struct IvfSlot {   // slot 0 holds the key itself (0: nothing yet — below every real key); slots 1 .. 63 do not exist
    __device__ __forceinline__ u64 key(u64 stored, int s) const { return s == 0 ? stored : ~0ull; }
    __device__ __forceinline__ float screen(u64 key) const { return __uint_as_float(score_from_sortkey(key)); }   // of key 0: a NaN, everything passes
};

// DIM > 0: 256 threads; DIM == 0: any dimension that is a multiple of 8, 64 / 128 / 256 threads by what fits the LDS
template <int DIM, int MODE>
__global__ __launch_bounds__(256) void ivf_assign_kernel(IvfAssignArgs a, int xstride, int qstride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int dim = DIM ? DIM : (int)a.dim;
    const int nthreads = (int)blockDim.x, rows_wg = (nthreads >> 6) * (int)kJoinTileRowsPerWave;
    float* xs = reinterpret_cast<float*>(smem);   // [rows_wg][xstride]
    float* qs = xs + (size_t)rows_wg * xstride;   // [kQC][qstride]
    const int tid = (int)threadIdx.x, lane = tid & 63, t = lane & 15;
    const int gid = tid >> 4;   // group of the workgroup
    const uint32_t tile_row0 = a.row0 + blockIdx.x * (uint32_t)rows_wg, row_end = a.row0 + a.nrows;
    const uint32_t nq = a.nlist;

    // the group's rows and whether they are assigned; a workgroup without a gated row has nothing to do
    bool act[kTR];
    int any = 0;
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
        const uint32_t row = tile_row0 + (uint32_t)(gid * kTR + r);
        act[r] = row < row_end && row_live(a.gate, row);
        any |= act[r] ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;

    load_row_tile(xs, a.slab, a.row_stride, false, dim, tile_row0, row_end, rows_wg, xstride, tid, nthreads);

    const IvfSlot pol;
    GroupLists<u64, IvfSlot> g;
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) g.slot[r][i] = 0ull;
    g.threshold_all(pol, t);

    const float* xr0 = xs + (size_t)(gid * kTR) * xstride + 2 * t;
    stream_chunks<DIM>(a.centroids, nq, dim, xr0, qs, xstride, qstride, tid, nthreads, t,
                       [&](f32x2(&acc)[kTR][kTQ], const float* xr, const float* qt, uint32_t q_first) {
        float s[kTR][kTQ];
        finish_tile<DIM, MODE, true, true>(acc, s, xr, qt, dim, xstride, qstride, t);
#pragma unroll
        for (int r = 0; r < kTR; ++r)
#pragma unroll
            for (int j = 0; j < kTQ; ++j) {
                // a centroid past the matrix's end is no candidate; the float compare only screens (NaN on either side passes)
                if (act[r] && q_first + (uint32_t)j < nq && !(s[r][j] < g.thrf[r])) {
                    const u64 key = ((u64)score_ord(__float_as_uint(s[r][j])) << 32) | (uint32_t)~(q_first + (uint32_t)j);
                    if (key > g.thr[r]) g.insert_row(r, pol, key, lane, t);
                }
            }
    });

#pragma unroll
    for (int r = 0; r < kTR; ++r)
        if (act[r] && t == 0) a.assign[tile_row0 + (uint32_t)(gid * kTR + r)] = ~(uint32_t)g.slot[r][0];
}

template <int DIM>
hipError_t assign_m(const IvfAssignArgs& a, const JoinTilePlan& p, hipStream_t stream) {
    if (a.hreduce == 2) return launch_join_tile(ivf_assign_kernel<DIM, 2>, a, p, stream);
    if (a.hreduce == 1) return launch_join_tile(ivf_assign_kernel<DIM, 1>, a, p, stream);
    return launch_join_tile(ivf_assign_kernel<DIM, 0>, a, p, stream);
}

__global__ __launch_bounds__(256) void ivf_count_changed_kernel(const uint32_t* __restrict__ assign, const uint32_t* __restrict__ prev,
                                                                const u64* __restrict__ gate, uint32_t n, u64* out) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    const int changed = r < n && row_live(gate, r) && assign[r] != prev[r];
    const int c = __syncthreads_count(changed);
    if (threadIdx.x == 0 && c) atomicAdd(reinterpret_cast<unsigned long long*>(out), (unsigned long long)c);
}

// a row outside every list (assign >= nlist) takes list nlist: key half 0, behind every list
__global__ __launch_bounds__(256) void ivf_list_keys_kernel(const uint32_t* __restrict__ assign, uint32_t n, uint32_t nlist, u64* __restrict__ keys) {
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n) return;
    const uint32_t a = assign[r], list = a < nlist ? a : nlist;
    keys[r] = ((u64)(nlist - list) << 32) | (uint32_t)~r;
}

// sorted[i]: ascending (list, row).  offsets[l] = the first position whose list is >= l; the thread at a boundary writes every l
// between its predecessor's list and its own, the last thread those behind its own.
__global__ __launch_bounds__(256) void ivf_list_emit_kernel(const u64* __restrict__ sorted, uint32_t n, uint32_t nlist, u64* __restrict__ offsets,
                                                            uint32_t* __restrict__ rows) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) return;
    const u64 e = sorted[i];
    const uint32_t list = nlist - (uint32_t)(e >> 32);
    const uint32_t first = i ? nlist - (uint32_t)(sorted[i - 1] >> 32) + 1u : 0u;
    for (uint32_t l = first; l <= list; ++l) offsets[l] = i;
    if (list < nlist) rows[i] = ~(uint32_t)e;
    if (i + 1 == n)
        for (uint32_t l = list + 1; l <= nlist; ++l) offsets[l] = n;
}

// One workgroup per list, lanes along the dimension so that a member's elements are read side by side; the sum of a (list,
// dimension) is one chain of dependent f64 adds in list_rows' order, eight members' loads in flight ahead of it.
__global__ __launch_bounds__(256) void ivf_update_kernel(IvfUpdateArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    double* mean = reinterpret_cast<double*>(smem);   // [dim]
    __shared__ double s_norm2;
    const uint32_t l = blockIdx.x, dim = a.dim;
    const u64 off = a.offsets[l], cnt = a.offsets[l + 1] - off;
    if (cnt == 0) return;   // (block-uniform) a list without members keeps its centroid
    const unsigned char* slab = reinterpret_cast<const unsigned char*>(a.slab);
    const uint32_t* members = a.list_rows + off;
    for (uint32_t d = threadIdx.x; d < dim; d += 256) {
        double s = 0.0;
        u64 i = 0;
        for (; i + 8 <= cnt; i += 8) {
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = (float)reinterpret_cast<const _Float16*>(slab + (size_t)members[i + u] * a.row_stride)[d];
#pragma unroll
            for (int u = 0; u < 8; ++u) s = s + (double)v[u];
        }
        for (; i < cnt; ++i) s = s + (double)(float)reinterpret_cast<const _Float16*>(slab + (size_t)members[i] * a.row_stride)[d];
        mean[d] = s / (double)cnt;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        double n2 = 0.0;
        for (uint32_t d = 0; d < dim; ++d) {
            const double p = mean[d] * mean[d];
            n2 = n2 + p;
        }
        s_norm2 = n2;
    }
    __syncthreads();
    const double n2 = s_norm2;
    if (!(n2 > 0.0) || !(n2 < __builtin_huge_val())) return;   // NaN, +inf, 0: the centroid stays
    const double norm = __builtin_sqrt(n2);
    for (uint32_t d = threadIdx.x; d < dim; d += 256) a.centroids[(size_t)l * dim + d] = (float)(mean[d] / norm);
}

// One workgroup per query: the k entries of each probed slot into LDS (kEmpty for a pair without a slot and for the padding up
// to a power of two), the block sort, the first k out.  kEmpty sorts behind every real entry (its row half is the greatest).
__global__ __launch_bounds__(256) void ivf_merge_kernel(IvfMergeArgs a, int np2) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    u64* buf = reinterpret_cast<u64*>(smem);   // [np2]
    const uint32_t q = blockIdx.x, k = a.k, total = a.nprobe * k;
    const int tid = (int)threadIdx.x;
    for (uint32_t i = tid; i < (uint32_t)np2; i += 256) {
        u64 e = kEmpty;
        if (i < total) {
            const uint32_t j = i / k, slot = a.qslots[(size_t)q * a.nprobe + j];
            if (slot != kIvfNoSlot) e = a.slot_lists[(size_t)slot * a.slot_stride + (i - j * k)];
        }
        buf[i] = e;
    }
    block_sort_desc_rt<256>(buf, np2, tid);   // (begins and ends with a barrier)
    int real = 0;   // k <= 256: one entry per thread
    if ((uint32_t)tid < k) {
        const u64 e = buf[tid];
        a.out_rows[(size_t)q * k + tid] = (uint32_t)e;
        a.out_scores[(size_t)q * k + tid] = __uint_as_float((uint32_t)(e >> 32));
        real = e != kEmpty;
    }
    const int count = __syncthreads_count(real);
    if (tid == 0) a.out_counts[q] = (uint32_t)count;
}

}  // namespace

bool ivf_assign_supported(uint32_t dim) {
    return dim >= 8 && dim % 8 == 0 && plan_join_tile(dim, 0, kIvfLdsBudget, {384, 256, 128, 64}).lds != 0;
}

// rows [row0, row0 + nrows) against the whole centroid matrix; dim % 8 == 0, 1 <= nlist
hipError_t launch_ivf_assign(const IvfAssignArgs& a, hipStream_t stream) {
    if (a.nrows == 0) return hipSuccess;
    if (a.nlist < 1 || a.nlist > kIvfMaxLists || a.dim < 8 || a.dim % 8 != 0 || (uint64_t)a.row0 + a.nrows > 0xfffffffeull) return hipErrorInvalidValue;
    const JoinTilePlan p = plan_join_tile(a.dim, 0, kIvfLdsBudget, {384, 256, 128, 64});
    if (p.lds == 0) return hipErrorInvalidValue;
    if (p.fixed) {
        if (a.dim == 384) return assign_m<384>(a, p, stream);
        if (a.dim == 256) return assign_m<256>(a, p, stream);
        if (a.dim == 128) return assign_m<128>(a, p, stream);
        return assign_m<64>(a, p, stream);
    }
    return assign_m<0>(a, p, stream);
}

hipError_t launch_ivf_count_changed(const uint32_t* assign, const uint32_t* prev, const u64* gate, uint32_t n, u64* out, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(ivf_count_changed_kernel, dim3((n + 255u) / 256u), dim3(256), 0, stream, assign, prev, gate, n, out);
    return hipGetLastError();
}

hipError_t launch_ivf_lists(const uint32_t* assign, uint32_t n, uint32_t nlist, u64* keys, u64* sorted, void* sort_temp, size_t sort_temp_bytes,
                            u64* offsets, uint32_t* rows, hipStream_t stream) {
    if (n == 0 || nlist < 1 || nlist > kIvfMaxLists || n > 0xfffffffeu) return hipErrorInvalidValue;
    const dim3 grid((n + 255u) / 256u), block(256);
    hipLaunchKernelGGL(ivf_list_keys_kernel, grid, block, 0, stream, assign, n, nlist, keys);
    // the key bits that can differ: the list half up to nlist, the row half below the highest bit of n - 1
    auto mask_of = [](uint32_t v) {
        uint32_t bits = 0;
        while (bits < 32u && (v >> bits) != 0) ++bits;
        return bits >= 32u ? 0xffffffffull : ((1ull << bits) - 1ull);
    };
    hipError_t e = sort_keys_desc(sort_temp, sort_temp_bytes, keys, sorted, (size_t)n, stream, (mask_of(nlist) << 32) | mask_of(n - 1));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ivf_list_emit_kernel, grid, block, 0, stream, (const u64*)sorted, n, nlist, offsets, rows);
    return hipGetLastError();
}

hipError_t launch_ivf_update(const IvfUpdateArgs& a, hipStream_t stream) {
    if (a.nlist == 0) return hipSuccess;
    if (a.nlist > kIvfMaxLists || a.dim < 1 || (size_t)a.dim * 8 > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_update_kernel, dim3(a.nlist), dim3(256), (size_t)a.dim * 8, stream, a);
    return hipGetLastError();
}

hipError_t launch_ivf_merge(const IvfMergeArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    const uint64_t total = (uint64_t)a.nprobe * a.k;
    if (a.nprobe < 1 || a.k < 1 || a.k > 256 || total > kIvfMergeMaxEntries) return hipErrorInvalidValue;
    int np2 = 64;
    while ((uint64_t)np2 < total) np2 <<= 1;
    const size_t lds = (size_t)np2 * 8;
    if (lds > 48 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(ivf_merge_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(ivf_merge_kernel, dim3(nq), dim3(256), lds, stream, a, np2);
    return hipGetLastError();
}

}  // namespace fsgpu

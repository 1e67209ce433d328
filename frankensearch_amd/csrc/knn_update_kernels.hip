// knn_update_kernels.hip — carrying the exact k-NN table across a compaction, a vacuum or deletes (include/fsgpu.h,
// fsgpu_index_update_knn_graph; vector_index_knn_update.cpp).
//
//   knn_update_inverse_kernel    new_to_old -> its inverse (old row -> current row)
//   knn_update_classify_kernel   per current row: dead / added / kept-clean / kept-dirty, and a kept-clean row's old list remapped
//                                into the working table as packed entries, sorted
//   knn_update_scatter_kernel    the lists of a search step (added and kept-dirty sources) into the working table
//   knn_update_join_kernel       kept-clean rows x added rows: the transposed exact join, the hot path
//   knn_update_output_kernel     the working table -> global ids and sims
//
// THE JOIN'S SCORE.  knn(x, m) scores target a against the query "row x widened to f32" with the slab's byte dot:
// dot_product_f16_bytes_f32 (simd.rs:361-446; leftover chunks before the tree) or dot_product_f32_bytes_f32 (simd.rs:581-702; after
// it), both with a FUSED tail.  The order of a dot's additions depends on the element index alone, so the kernel may hold x in LDS,
// stream a past it on join_tile.hpp's tile (the mapping of lanes to the dot's chains is described there) and still produce
// score(x, a) bit for bit.
//
// A row's running list (m <= 63) holds packed entries, initialised from the working table; its m-th sortkey is the threshold, an
// exact compare of (score, row).  At the end the list is rank-sorted with shuffles inside the group and written back.  Rows of the
// other classes are loaded but never scored into or written.
#include "join_tile.hpp"

namespace fsgpu {

namespace {

__global__ __launch_bounds__(256) void knn_update_inverse_kernel(const uint32_t* new_to_old, uint64_t n, uint64_t old_len, uint32_t* inv) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= n) return;
    const uint32_t p = new_to_old[x];
    if (p < old_len) inv[p] = (uint32_t)x;
}

// One wave per current row, one lane per column, four rows per block.
__global__ __launch_bounds__(256) void knn_update_classify_kernel(KnnUpdClassifyArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t x = (uint64_t)blockIdx.x * 4u + (threadIdx.x >> 6);
    if (x >= a.n) return;
    const uint32_t m = a.m;
    const bool live = row_live(a.live, x);
    uint32_t pred = a.new_to_old ? a.new_to_old[x] : (x < a.old_len ? (uint32_t)x : kKnnPadRow);
    if (pred >= a.old_len) pred = kKnnPadRow;
    uint32_t id = kKnnPadRow;
    float sim = 0.0f;
    if (live && pred != kKnnPadRow && lane < m) {
        id = a.old_rows[(uint64_t)pred * m + lane];
        sim = a.old_sims[(uint64_t)pred * m + lane];
    }
    // the list ends at its first pad; what a hostile table holds behind it is not read as entries
    const unsigned long long pads = __ballot(lane < m && id == kKnnPadRow);
    const uint32_t len = pads ? (uint32_t)(__ffsll(pads) - 1) : m;
    uint32_t y = kKnnPadRow;
    bool dropped = false;
    if (lane < len) {
        const uint32_t o = id - a.old_row_base;
        if (id < a.old_row_base || o >= a.old_len) {
            dropped = true;
        } else {
            y = a.inv ? a.inv[o] : o;
            if (y == kKnnPadRow || y >= a.n || !row_live(a.live, y)) dropped = true;
        }
    }
    const bool any_dropped = __ballot(dropped) != 0ull;
    uint8_t cls;
    if (!live) cls = kKnnUpdDead;
    else if (len == 0) cls = kKnnUpdAdded;
    else cls = (any_dropped || a.all_dirty) ? kKnnUpdDirty : kKnnUpdClean;
    if (lane == 0) a.cls[x] = cls;
    u64* w = a.work + x * m;
    if (cls != kKnnUpdClean) {
        if (lane < m) w[lane] = kEmpty;
        return;
    }
    // after a monotone remap the old order is the total order already; nothing is assumed: rank-sort the wave's entries
    const u64 e = lane < len ? pack(sim, y) : kEmpty;
    const u64 key = sortkey(e);
    uint32_t rank = 0;
    for (uint32_t s = 0; s < m; ++s) {
        const u64 other = __shfl(key, (int)s);
        rank += (other > key || (other == key && s < lane)) ? 1u : 0u;
    }
    if (lane < m) w[rank] = e;
}

// One wave per source of the step, four per block: lane l carries entry l of its list.
__global__ __launch_bounds__(256) void knn_update_scatter_kernel(KnnUpdScatterArgs a) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t s = blockIdx.x * 4u + (threadIdx.x >> 6);
    if (s >= a.n || lane >= a.m) return;
    const uint32_t src = a.src[s] - a.row_base;
    if (src >= a.nrows) return;
    const uint32_t row = a.rows[(uint64_t)s * a.m + lane];
    const uint32_t local = row - a.row_base;
    const bool real = row != kKnnPadRow && row >= a.row_base && local < a.nrows;
    a.work[(uint64_t)src * a.m + lane] = real ? pack(a.sims[(uint64_t)s * a.m + lane], local) : kEmpty;
}

// ---- the join ----
struct UpdSlots {   // a slot holds a packed entry (kEmpty: none) and competes with its sortkey; slots >= m do not exist
    int m;
    __device__ __forceinline__ u64 key(u64 packed, int s) const { return s < m ? sortkey(packed) : ~0ull; }
    __device__ __forceinline__ float screen(u64 key) const { return __uint_as_float(score_from_sortkey(key)); }
};

// DIM > 0: 256 threads; DIM == 0: any dimension up to kKnnUpdMaxDim, 64 / 128 / 256 threads by what fits the LDS
template <bool F32, int DIM, int MODE>
__global__ __launch_bounds__(256) void knn_update_join_kernel(KnnUpdJoinArgs a, int xstride, int qstride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int dim = DIM ? DIM : (int)a.dim;
    const int nthreads = (int)blockDim.x, rows_wg = (nthreads >> 6) * (int)kKnnUpdRowsPerWave;
    float* xs = reinterpret_cast<float*>(smem);            // [rows_wg][xstride]
    float* qs = xs + (size_t)rows_wg * xstride;            // [kQC][qstride]
    const int tid = (int)threadIdx.x, lane = tid & 63, t = lane & 15;
    const int gid = tid >> 4;   // group of the workgroup
    const uint32_t tile_row0 = a.row0 + blockIdx.x * (uint32_t)rows_wg, row_end = a.row0 + a.nrows;
    const uint32_t nq = a.n_added;
    const int m = (int)a.m;

    // the group's rows and whether they are scored into; a workgroup without a kept-clean row has nothing to do
    bool act[kTR];
    int any = 0;
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
        const uint32_t row = tile_row0 + (uint32_t)(gid * kTR + r);
        act[r] = row < row_end && a.cls[row] == kKnnUpdClean;
        any |= act[r] ? 1 : 0;
    }
    if (!__syncthreads_or(any)) return;

    load_row_tile(xs, a.slab, a.row_stride, F32, dim, tile_row0, row_end, rows_wg, xstride, tid, nthreads);

    const UpdSlots pol{m};
    GroupLists<u64, UpdSlots> g;
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
        const size_t at = (size_t)(tile_row0 + (uint32_t)(gid * kTR + r)) * (size_t)m;
#pragma unroll
        for (int i = 0; i < 4; ++i) g.slot[r][i] = (act[r] && t + 16 * i < m) ? a.work[at + (size_t)(t + 16 * i)] : kEmpty;
    }
    g.threshold_all(pol, t);

    const float* xr0 = xs + (size_t)(gid * kTR) * xstride + 2 * t;
    stream_chunks<DIM>(a.added, nq, dim, xr0, qs, xstride, qstride, tid, nthreads, t,
                       [&](f32x2(&acc)[kTR][kTQ], const float* xr, const float* qt, uint32_t q_first) {
        float s[kTR][kTQ];
        finish_tile<DIM, MODE, !F32, true>(acc, s, xr, qt, dim, xstride, qstride, t);
#pragma unroll
        for (int r = 0; r < kTR; ++r)
#pragma unroll
            for (int j = 0; j < kTQ; ++j) {
                // an added row past the block's end is no candidate; the float compare only screens (NaN on either side passes)
                if (act[r] && q_first + (uint32_t)j < nq && !(s[r][j] < g.thrf[r])) {
                    const u64 packed = pack(s[r][j], a.added_rows[q_first + (uint32_t)j]);
                    if (sortkey(packed) > g.thr[r]) g.insert_row(r, pol, packed, lane, t);
                }
            }
    });

    // per kept-clean row: the m entries rank-sorted inside the group (best first; the pads tie and keep their slot order)
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
        if (!act[r]) continue;   // (uniform over the group)
        u64 key[4];
        int rank[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) key[i] = sortkey(g.slot[r][i]);
#pragma unroll 1
        for (int s = 0; s < m; ++s) {   // slot s lives in lane s & 15 of the group, register s >> 4
            const int i = s >> 4;
            const u64 held = i == 0 ? key[0] : i == 1 ? key[1] : i == 2 ? key[2] : key[3];
            const u64 other = __shfl(held, s & 15, 16);
#pragma unroll
            for (int i2 = 0; i2 < 4; ++i2) rank[i2] += (other > key[i2] || (other == key[i2] && s < t + 16 * i2)) ? 1 : 0;
        }
        u64* w = a.work + (size_t)(tile_row0 + (uint32_t)(gid * kTR + r)) * (size_t)m;
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t + 16 * i < m) w[rank[i]] = g.slot[r][i];
    }
}

// One entry per thread; a block's count of "kept-clean list entry that is an added row" goes to join_entries[block].
__global__ __launch_bounds__(256) void knn_update_output_kernel(KnnUpdOutputArgs a) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x, total = a.n * a.m;
    int counted = 0;
    if (idx < total) {
        const u64 e = a.work[idx];
        const uint32_t y = (uint32_t)e;
        const bool real = e != kEmpty && y < a.n;
        a.out_rows[idx] = real ? a.row_base + y : kKnnPadRow;
        a.out_sims[idx] = real ? __uint_as_float((uint32_t)(e >> 32)) : 0.0f;
        counted = real && a.cls[idx / a.m] == kKnnUpdClean && a.cls[y] == kKnnUpdAdded;
    }
    const int c = __syncthreads_count(counted);
    if (threadIdx.x == 0) a.join_entries[blockIdx.x] = (uint32_t)c;
}

template <bool F32, int DIM>
hipError_t join_m(const KnnUpdJoinArgs& a, const JoinTilePlan& p, hipStream_t stream) {
    if (a.hreduce == 2) return launch_join_tile(knn_update_join_kernel<F32, DIM, 2>, a, p, stream);
    if (a.hreduce == 1) return launch_join_tile(knn_update_join_kernel<F32, DIM, 1>, a, p, stream);
    return launch_join_tile(knn_update_join_kernel<F32, DIM, 0>, a, p, stream);
}

template <bool F32>
hipError_t join_d(const KnnUpdJoinArgs& a, const JoinTilePlan& p, hipStream_t stream) {
    if (p.fixed) {
        if (a.dim == 384) return join_m<F32, 384>(a, p, stream);
        if (a.dim == 256) return join_m<F32, 256>(a, p, stream);
        if (a.dim == 128) return join_m<F32, 128>(a, p, stream);
        return join_m<F32, 64>(a, p, stream);
    }
    return join_m<F32, 0>(a, p, stream);
}

}  // namespace

hipError_t launch_knn_update_inverse(const uint32_t* new_to_old, uint64_t n, uint64_t old_len, uint32_t* inv, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    hipLaunchKernelGGL(knn_update_inverse_kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, stream, new_to_old, n, old_len, inv);
    return hipGetLastError();
}

hipError_t launch_knn_update_classify(const KnnUpdClassifyArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.m < 1 || a.m > kKnnMaxM || a.n > 0xfffffffeull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_update_classify_kernel, dim3((uint32_t)((a.n + 3) / 4)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_knn_update_scatter(const KnnUpdScatterArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.m < 1 || a.m > kKnnMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_update_scatter_kernel, dim3((a.n + 3u) / 4u), dim3(256), 0, stream, a);
    return hipGetLastError();
}

// rows [row0, row0 + nrows) against one block of added rows; 1 <= m <= kKnnMaxM, 1 <= dim <= kKnnUpdMaxDim
hipError_t launch_knn_update_join(const KnnUpdJoinArgs& a, hipStream_t stream) {
    if (a.nrows == 0 || a.n_added == 0) return hipSuccess;
    if (a.m < 1 || a.m > kKnnMaxM || a.dim < 1 || a.dim > kKnnUpdMaxDim || (uint64_t)a.row0 + a.nrows > 0xfffffffeull) return hipErrorInvalidValue;
    const JoinTilePlan p = plan_join_tile(a.dim, 0, kKnnUpdLdsBudget, {384, 256, 128, 64});
    if (p.lds == 0) return hipErrorInvalidValue;   // (the budget leaves room for the block vote's few static bytes)
    return a.slab_f32 ? join_d<true>(a, p, stream) : join_d<false>(a, p, stream);
}

uint32_t knn_update_output_blocks(uint64_t n, uint32_t m) { return (uint32_t)((n * m + 255) / 256); }

hipError_t launch_knn_update_output(const KnnUpdOutputArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.m < 1 || a.m > kKnnMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_update_output_kernel, dim3(knn_update_output_blocks(a.n, a.m)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu

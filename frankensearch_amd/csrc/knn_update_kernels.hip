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
// dot_product_f16_bytes_f32 (simd.rs:361-446) or dot_product_f32_bytes_f32 (simd.rs:581-702).  Both are four 8-lane accumulators over
// groups of 32 elements (accumulator a, lane l takes element 32 g + 8 a + l; a separate multiply and add — this file is compiled with
// -ffp-contract=off), (acc0 + acc1) + (acc2 + acc3), reduce_add in the index's horizontal order and a FUSED multiply-add per element
// of the last dim % 8.  They differ in the leftover 8-element chunks: the f16 dot adds them into acc0 BEFORE the tree, the f32 dot
// to the tree's sum after it.  Every product is f32(x_e) * f32(a_e), which commutes, and the order of the additions depends on the
// element index alone: the kernel may hold x in LDS and stream a past it and still produce score(x, a) bit for bit.
//
// MAPPING: hubness_kernels.hip's.  A dot is 32 independent chains; sixteen lanes form a group, lane t owns the adjacent chains 2 t and
// 2 t + 1 (a = t >> 2, l = 2 (t & 3) and + 1): one 8-byte LDS read per operand and group of 32, packed f32 multiply / add on natural
// register pairs.  A group keeps a register tile of 4 rows x 8 added rows.  The tree is two DPP steps inside the 16-lane row, the
// horizontal add two or three quad steps; every lane of the group ends with the same bits.  A workgroup of W waves owns 16 W rows,
// widened to f32 in LDS once, and streams the block of added rows past them in chunks of 16, in the same order in every workgroup.
// A row's running list lives in the registers of its group (m <= 63 < 64 = 16 lanes x 4 slots) as packed entries, initialised from
// the working table; its m-th sortkey is the threshold (a float pre-check, then the exact compare of (score, row)); a candidate that
// beats it replaces it and the new threshold is a 16-lane DPP reduction.  At the end the list is rank-sorted with shuffles inside
// the group and written back.  A row is owned by one group: no atomics, and rows of the other classes are loaded but never scored
// into or written.
#include "kernels.hpp"
#include "device_util.hpp"

namespace fsgpu {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kQC = (int)kKnnUpdChunk;   // added rows per LDS chunk
constexpr int kTR = 4, kTQ = 8;          // the register tile of a 16-lane group: rows x added rows

__device__ __forceinline__ bool upd_live(const u64* live, uint64_t r) { return !live || ((live[r >> 6] >> (r & 63u)) & 1ull); }

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
    const bool live = upd_live(a.live, x);
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
            if (y == kKnnPadRow || y >= a.n || !upd_live(a.live, y)) dropped = true;
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
// lane t ^ 4 inside a row of 16: the lower quad of each pair takes lane + 4, the upper lane - 4 (hubness_kernels.hip)
__device__ __forceinline__ int row_xor4_i(int x) {
    int t = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xF, 0x5, false);
    return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);
}
__device__ __forceinline__ int row_xor8_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false); }   // row_ror:8
__device__ __forceinline__ int quad_xor1_i(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ int quad_xor2_i(int x) { return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true); }
__device__ __forceinline__ float row_xor4(float v) { return __int_as_float(row_xor4_i(__float_as_int(v))); }
__device__ __forceinline__ float row_xor8(float v) { return __int_as_float(row_xor8_i(__float_as_int(v))); }
__device__ __forceinline__ float quad_pair_lo(float v) {   // quad_perm [0,0,2,2]
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xA0, 0xF, 0xF, true));
}
__device__ __forceinline__ float quad_pair_hi(float v) {   // quad_perm [1,1,3,3]
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xF5, 0xF, 0xF, true));
}
#define FSGPU_UPD_MIN_STEP(fn)                                                                              \
    {                                                                                                       \
        const u64 o = ((u64)(uint32_t)fn((int)(uint32_t)(v >> 32)) << 32) | (uint32_t)fn((int)(uint32_t)v); \
        v = o < v ? o : v;                                                                                  \
    }
__device__ __forceinline__ u64 group_min16(u64 v) {   // the minimum over the 16 lanes of a group, in every one of them
    FSGPU_UPD_MIN_STEP(quad_xor1_i)
    FSGPU_UPD_MIN_STEP(quad_xor2_i)
    FSGPU_UPD_MIN_STEP(row_xor4_i)
    FSGPU_UPD_MIN_STEP(row_xor8_i)
    return v;
}
#undef FSGPU_UPD_MIN_STEP

// wide::f32x8::reduce_add of v[0..8) held as (v[2 p], v[2 p + 1]) by lane p = t & 3 of every quad (hubness_kernels.hip):
// MODE 0 = SSE2 build order, 1 = AVX order, 2 = two sequential 4-lane sums
template <int MODE>
__device__ __forceinline__ float hreduce_pairs(f32x2 v) {
    if (MODE == 2) {
        const float e0x = quad_pair_lo(v.x), e0y = quad_pair_lo(v.y), e1x = quad_pair_hi(v.x), e1y = quad_pair_hi(v.y);
        const float w = ((e0x + e0y) + e1x) + e1y;
        return w + quad_xor2(w);
    }
    if (MODE == 1) {
        const float ux = v.x + quad_xor2(v.x), uy = v.y + quad_xor2(v.y);
        const float lo = ux + quad_xor1(ux), hi = uy + quad_xor1(uy);
        return lo + hi;
    }
    const float ux = v.x + quad_xor1(v.x), uy = v.y + quad_xor1(v.y);
    const float w = ux + uy;
    return w + quad_xor2(w);
}

// The running lists of the group's kTR rows: slot (t + 16 i) of row r in slot[r][i] as a packed entry (kEmpty: none).  Slots >= m do
// not exist: they count as the greatest key and are never replaced.  thr[r] = the least sortkey over the row's m slots.
struct GroupLists {
    u64 slot[kTR][4];
    u64 thr[kTR];
    float thrf[kTR];
};

__device__ __forceinline__ u64 slot_key(u64 packed, int s, int m) { return s < m ? sortkey(packed) : ~0ull; }

template <int R>
__device__ __forceinline__ void upd_threshold(GroupLists& g, int t, int m) {
    u64 v = slot_key(g.slot[R][0], t, m);
#pragma unroll
    for (int i = 1; i < 4; ++i) {
        const u64 k = slot_key(g.slot[R][i], t + 16 * i, m);
        v = k < v ? k : v;
    }
    v = group_min16(v);
    g.thr[R] = v;
    g.thrf[R] = __uint_as_float(score_from_sortkey(v));
}

template <int R>
__device__ __forceinline__ void upd_insert(GroupLists& g, u64 packed, int lane, int t, int m) {
    bool done = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 b = __ballot(!done && slot_key(g.slot[R][i], t + 16 * i, m) == g.thr[R]);
        const uint32_t mine = (uint32_t)(b >> (lane & 48)) & 0xffffu;   // this group's 16 lanes
        if (!done && mine) {
            if (t == __ffs((int)mine) - 1) g.slot[R][i] = packed;
            done = true;
        }
    }
    upd_threshold<R>(g, t, m);
}

// tree, leftovers, horizontal add and tail of the tile in the byte dot's order, then the threshold-gated inserts
template <bool F32, int DIM, int MODE>
__device__ __forceinline__ void upd_finish_tile(f32x2 (&acc)[kTR][kTQ], GroupLists& g, const bool (&act)[kTR], const float* xr, const float* qt,
                                                int dim, int xstride, int qstride, uint32_t q_first, const KnnUpdJoinArgs& a, int lane, int t) {
    const int chunks = dim >> 3, groups = chunks >> 2;
    const int p2 = 2 * (t & 3);
    const int m = (int)a.m;
    // every phase keeps the tile's (r, j) loops innermost and fully unrolled, so that the accumulators stay in registers
    if (DIM == 0 && !F32) {
        if (t < 4) {   // the f16 dot: leftover chunks go into accumulator 0 BEFORE the tree (simd.rs:419-431); 2 t = p2 here
            for (int c = 4 * groups; c < chunks; ++c) {
                f32x2 x[kTR], q[kTQ];
#pragma unroll
                for (int r = 0; r < kTR; ++r) x[r] = *reinterpret_cast<const f32x2*>(xr + r * xstride + 8 * c);
#pragma unroll
                for (int j = 0; j < kTQ; ++j) q[j] = *reinterpret_cast<const f32x2*>(qt + j * qstride + 8 * c + p2);
#pragma unroll
                for (int r = 0; r < kTR; ++r)
#pragma unroll
                    for (int j = 0; j < kTQ; ++j) {
                        const f32x2 p = x[r] * q[j];
                        acc[r][j] = acc[r][j] + p;
                    }
            }
        }
    }
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int j = 0; j < kTQ; ++j) {
            f32x2 u = acc[r][j];
            u.x = u.x + row_xor4(u.x);   // acc0 + acc1 | acc2 + acc3
            u.y = u.y + row_xor4(u.y);
            u.x = u.x + row_xor8(u.x);   // (acc0 + acc1) + (acc2 + acc3)
            u.y = u.y + row_xor8(u.y);
            acc[r][j] = u;
        }
    if (DIM == 0 && F32) {
        for (int c = 4 * groups; c < chunks; ++c) {   // the f32 dot: leftover chunks join AFTER the tree (simd.rs:660-672)
            f32x2 x[kTR], q[kTQ];
#pragma unroll
            for (int r = 0; r < kTR; ++r) x[r] = *reinterpret_cast<const f32x2*>(xr + r * xstride - 2 * t + 8 * c + p2);
#pragma unroll
            for (int j = 0; j < kTQ; ++j) q[j] = *reinterpret_cast<const f32x2*>(qt + j * qstride + 8 * c + p2);
#pragma unroll
            for (int r = 0; r < kTR; ++r)
#pragma unroll
                for (int j = 0; j < kTQ; ++j) {
                    const f32x2 p = x[r] * q[j];
                    acc[r][j] = acc[r][j] + p;
                }
        }
    }
    float s[kTR][kTQ];
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int j = 0; j < kTQ; ++j) s[r][j] = hreduce_pairs<MODE>(acc[r][j]);
    if (DIM == 0) {
        for (int i = chunks * 8; i < dim; ++i) {   // the fused tail of both byte dots
            float x[kTR], q[kTQ];
#pragma unroll
            for (int r = 0; r < kTR; ++r) x[r] = xr[r * xstride - 2 * t + i];
#pragma unroll
            for (int j = 0; j < kTQ; ++j) q[j] = qt[j * qstride + i];
#pragma unroll
            for (int r = 0; r < kTR; ++r)
#pragma unroll
                for (int j = 0; j < kTQ; ++j) s[r][j] = __builtin_fmaf(x[r], q[j], s[r][j]);
        }
    }
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
#pragma unroll
        for (int j = 0; j < kTQ; ++j) {
            // an added row past the block's end is no candidate; the float compare only screens (NaN on either side passes)
            if (act[r] && q_first + (uint32_t)j < a.n_added && !(s[r][j] < g.thrf[r])) {
                const u64 packed = pack(s[r][j], a.added_rows[q_first + (uint32_t)j]);
                if (sortkey(packed) > g.thr[r]) {
                    if (r == 0) upd_insert<0>(g, packed, lane, t, m);
                    if (r == 1) upd_insert<1>(g, packed, lane, t, m);
                    if (r == 2) upd_insert<2>(g, packed, lane, t, m);
                    if (r == 3) upd_insert<3>(g, packed, lane, t, m);
                }
            }
        }
    }
}

// DIM > 0: compile-time dimension (a multiple of 32), 256 threads, the next chunk of added rows prefetched into registers during the
// arithmetic.  DIM == 0: any dimension up to kKnnUpdMaxDim, 64 / 128 / 256 threads by what fits the LDS.
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

    // the tile's rows, widened to f32 (exact for f16); rows past the end are zeros.  Loads are clamped to the last row instead of
    // predicated, and four are in flight per thread (hubness_kernels.hip).
    const unsigned char* slab = reinterpret_cast<const unsigned char*>(a.slab);
    const bool vec = (a.row_stride & 15u) == 0 && (dim & 7) == 0 && (reinterpret_cast<uintptr_t>(a.slab) & 15u) == 0;
    if (vec) {
        const int cpr = dim >> 3, nchunks = rows_wg * cpr;   // 8-element chunks: 16 bytes of f16, 32 of f32
        for (int base = 0; base < nchunks; base += 4 * nthreads) {
            u32x4 lo[4], hi[4];
            int at[4];
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + tid + u * nthreads;
                const int idc = idx < nchunks ? idx : 0;
                const int r = idc / cpr, c = idc - r * cpr;
                const uint32_t row = tile_row0 + (uint32_t)r;
                const unsigned char* p = slab + (size_t)(row < row_end ? row : row_end - 1) * a.row_stride;
                at[u] = idx < nchunks ? (row < row_end ? r * xstride + 8 * c : -(r * xstride + 8 * c) - 2) : -1;
                if (F32) {
                    lo[u] = *reinterpret_cast<const u32x4*>(p + (size_t)c * 32);
                    hi[u] = *reinterpret_cast<const u32x4*>(p + (size_t)c * 32 + 16);
                } else {
                    lo[u] = *reinterpret_cast<const u32x4*>(p + (size_t)c * 16);
                    hi[u] = lo[u];
                }
            }
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                if (at[u] == -1) continue;
                float4 v0, v1;
                if (at[u] < 0) {   // a row past the end
                    v0 = v1 = make_float4(0.f, 0.f, 0.f, 0.f);
                } else if (F32) {
                    v0 = __builtin_bit_cast(float4, lo[u]);
                    v1 = __builtin_bit_cast(float4, hi[u]);
                } else {
                    const half8 h = __builtin_bit_cast(half8, lo[u]);
                    v0 = make_float4((float)h[0], (float)h[1], (float)h[2], (float)h[3]);
                    v1 = make_float4((float)h[4], (float)h[5], (float)h[6], (float)h[7]);
                }
                float* dst = xs + (at[u] < 0 ? -(at[u] + 2) : at[u]);
                *reinterpret_cast<float4*>(dst) = v0;
                *reinterpret_cast<float4*>(dst + 4) = v1;
            }
        }
    } else {
#pragma unroll 4
        for (int idx = tid; idx < rows_wg * dim; idx += nthreads) {
            const int r = idx / dim, e = idx - r * dim;
            const uint32_t row = tile_row0 + (uint32_t)r;
            const unsigned char* p = slab + (size_t)(row < row_end ? row : row_end - 1) * a.row_stride;
            const float v = F32 ? reinterpret_cast<const float*>(p)[e] : (float)reinterpret_cast<const _Float16*>(p)[e];
            xs[r * xstride + e] = row < row_end ? v : 0.0f;
        }
    }

    GroupLists g;
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
        const size_t at = (size_t)(tile_row0 + (uint32_t)(gid * kTR + r)) * (size_t)m;
#pragma unroll
        for (int i = 0; i < 4; ++i) g.slot[r][i] = (act[r] && t + 16 * i < m) ? a.work[at + (size_t)(t + 16 * i)] : kEmpty;
    }
    upd_threshold<0>(g, t, m);
    upd_threshold<1>(g, t, m);
    upd_threshold<2>(g, t, m);
    upd_threshold<3>(g, t, m);

    constexpr int NPF = DIM ? kQC * DIM / 256 : 1;
    float pf[NPF];
    const size_t q_total = (size_t)nq * dim;
    if (DIM) {   // (loads past the block's end are clamped, not predicated; the store below zeroes them)
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const size_t o = (size_t)(tid + 256 * i);
            pf[i] = a.added[o < q_total ? o : q_total - 1];
        }
    }
    const float* xr = xs + (size_t)(gid * kTR) * xstride + 2 * t;
    const int groups = dim >> 5;

    for (uint32_t q0 = 0; q0 < nq; q0 += kQC) {
        __syncthreads();   // the previous chunk has been read by every group
        if (DIM) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) qs[tid + 256 * i] = (size_t)q0 * dim + (size_t)(tid + 256 * i) < q_total ? pf[i] : 0.0f;
        } else {
            for (int idx = tid; idx < kQC * dim; idx += nthreads) {
                const int j = idx / dim, e = idx - j * dim;
                qs[j * qstride + e] = q0 + (uint32_t)j < nq ? a.added[(size_t)(q0 + j) * dim + e] : 0.0f;
            }
        }
        __syncthreads();
        if (DIM) {
            const size_t base = (size_t)(q0 + kQC) * dim;
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const size_t o = base + (size_t)(tid + 256 * i);
                pf[i] = a.added[o < q_total ? o : q_total - 1];
            }
        }
#pragma unroll 1
        for (int jt = 0; jt < kQC; jt += kTQ) {
            if (q0 + (uint32_t)jt >= nq) break;
            const float* qt = qs + (size_t)jt * qstride;
            f32x2 acc[kTR][kTQ];
#pragma unroll
            for (int r = 0; r < kTR; ++r)
#pragma unroll
                for (int j = 0; j < kTQ; ++j) acc[r][j] = f32x2{0.0f, 0.0f};
#pragma unroll 2
            for (int gr = 0; gr < groups; ++gr) {
                f32x2 x[kTR], q[kTQ];
#pragma unroll
                for (int r = 0; r < kTR; ++r) x[r] = *reinterpret_cast<const f32x2*>(xr + r * xstride + 32 * gr);
#pragma unroll
                for (int j = 0; j < kTQ; ++j) q[j] = *reinterpret_cast<const f32x2*>(qt + j * qstride + 32 * gr + 2 * t);
#pragma unroll
                for (int r = 0; r < kTR; ++r)
#pragma unroll
                    for (int j = 0; j < kTQ; ++j) {
                        const f32x2 p = x[r] * q[j];   // a multiply and an add, never an fma
                        acc[r][j] = acc[r][j] + p;
                    }
            }
            upd_finish_tile<F32, DIM, MODE>(acc, g, act, xr, qt, dim, xstride, qstride, q0 + (uint32_t)jt, a, lane, t);
        }
    }

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

template <bool F32, int DIM, int MODE>
hipError_t join_t(const KnnUpdJoinArgs& a, int waves, int xstride, int qstride, size_t lds, hipStream_t stream) {
    auto kern = knn_update_join_kernel<F32, DIM, MODE>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const uint32_t rows_wg = (uint32_t)waves * kKnnUpdRowsPerWave;
    const uint32_t grid = (a.nrows + rows_wg - 1) / rows_wg;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), lds, stream, a, xstride, qstride);
    return hipGetLastError();
}

template <bool F32, int DIM>
hipError_t join_m(const KnnUpdJoinArgs& a, int waves, int xstride, int qstride, size_t lds, hipStream_t stream) {
    if (a.hreduce == 2) return join_t<F32, DIM, 2>(a, waves, xstride, qstride, lds, stream);
    if (a.hreduce == 1) return join_t<F32, DIM, 1>(a, waves, xstride, qstride, lds, stream);
    return join_t<F32, DIM, 0>(a, waves, xstride, qstride, lds, stream);
}

template <bool F32>
hipError_t join_d(const KnnUpdJoinArgs& a, int waves, int xstride, int qstride, size_t lds, hipStream_t stream) {
    if (waves == 4) {
        if (a.dim == 384) return join_m<F32, 384>(a, 4, xstride, qstride, lds, stream);
        if (a.dim == 256) return join_m<F32, 256>(a, 4, xstride, qstride, lds, stream);
        if (a.dim == 128) return join_m<F32, 128>(a, 4, xstride, qstride, lds, stream);
        if (a.dim == 64) return join_m<F32, 64>(a, 4, xstride, qstride, lds, stream);
    }
    return join_m<F32, 0>(a, waves, xstride, qstride, lds, stream);
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
    // row stride in LDS: = 8 (mod 16) floats, so that the two groups of a half-wave (rows 4 apart) read disjoint halves of the
    // 64 banks with ds_read_b64; the added rows are a broadcast (hubness_kernels.hip)
    const int xstride = (int)((a.dim + 15u) & ~15u) + 8;
    const bool fixed = a.dim == 384 || a.dim == 256 || a.dim == 128 || a.dim == 64;
    const int qstride = fixed ? (int)a.dim : (int)((a.dim + 1u) & ~1u);
    auto lds_of = [&](int waves) { return ((size_t)waves * kKnnUpdRowsPerWave * xstride + (size_t)kKnnUpdChunk * qstride) * 4; };
    int waves = 4;
    while (waves > 1 && lds_of(waves) > kKnnUpdLdsBudget) waves >>= 1;
    const size_t lds = lds_of(waves);
    if (lds > kKnnUpdLdsBudget) return hipErrorInvalidValue;   // (the budget leaves room for the block vote's few static bytes)
    return a.slab_f32 ? join_d<true>(a, waves, xstride, qstride, lds, stream) : join_d<false>(a, waves, xstride, qstride, lds, stream);
}

uint32_t knn_update_output_blocks(uint64_t n, uint32_t m) { return (uint32_t)((n * m + 255) / 256); }

hipError_t launch_knn_update_output(const KnnUpdOutputArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (a.m < 1 || a.m > kKnnMaxM) return hipErrorInvalidValue;
    hipLaunchKernelGGL(knn_update_output_kernel, dim3(knn_update_output_blocks(a.n, a.m)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu

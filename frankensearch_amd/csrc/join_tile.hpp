// join_tile.hpp — the transposed exact join: a tile of slab ROWS held in LDS, a block of f32 vectors (queries, added rows) streamed
// past it, every (row, vector) dot product reproduced bit for bit, and per row a running list of the best in registers.  Shared
// by hubness_kernels.hip and knn_update_kernels.hip; each keeps its own key, candidate gate and epilogue.
//
// THE DOTS.  The index's three CPU dots (simd.rs) are four 8-lane accumulators over groups of 32 elements (accumulator a, lane l
// takes element 32 g + 8 a + l; a separate multiply and add — both files are compiled with -ffp-contract=off), the tree
// (acc0 + acc1) + (acc2 + acc3), reduce_add in the index's horizontal order (MODE), then the last dim % 8 elements one by one.
// They differ in two places, finish_tile's two flags: the leftover 8-element chunks go into acc0 BEFORE the tree or to the tree's
// sum AFTER it, and the tail is a FUSED multiply-add or a separate multiply and add:
//     dot_product_f32_f32        (simd.rs:134-222)   after the tree, unfused     hubness
//     dot_product_f16_bytes_f32  (simd.rs:361-446)   before the tree, fused      the update's join on an f16 slab
//     dot_product_f32_bytes_f32  (simd.rs:581-702)   after the tree, fused       the update's join on an f32 slab
// Every product is f32(x_e) * f32(q_e), which commutes, and the order of the additions depends on the element index alone.
//
// MAPPING.  A dot is 32 independent chains (chain c = 8 a + l holds elements c, 32 + c, 64 + c, ...), each sequential over the
// groups, followed by a fixed tree — so lanes that own chains need no reassociation.  Sixteen lanes form a group; lane t owns the
// ADJACENT chains 2 t and 2 t + 1 (a = t >> 2, l = 2 (t & 3) and + 1), i.e. one 8-byte LDS read per operand and group of 32, and
// the packed f32 multiply / add work on natural register pairs.  A group keeps a register tile of 4 rows x 8 streamed vectors (64
// accumulators per lane; 12 ds_read_b64 per 64 packed multiply-adds).  The tree is two DPP steps inside the 16-lane row (t ^ 4:
// acc0 + acc1 and acc2 + acc3; t ^ 8: their sum), the horizontal add two or three quad steps; every lane of the group ends with
// the same bits.  A workgroup of W waves owns 16 W rows (4 per group), widened to f32 in LDS once, and streams the block past them
// in chunks of 16 vectors, in the same order in every workgroup (the block is served from L2 / the Infinity Cache).  A row's
// running list lives in the registers of its group (at most 64 = 16 lanes x 4 slots) as integer keys; a score is inserted only
// when it beats the list's least key (a float pre-check, then the exact compare), replacing it, and the new least key is a 16-lane
// DPP reduction.  A row is owned by one group: no atomics.
#pragma once

#include <initializer_list>

#include "kernels.hpp"
#include "device_util.hpp"

namespace fsgpu {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kQC = (int)kJoinTileChunk;   // streamed vectors per LDS chunk
constexpr int kTR = 4, kTQ = 8;            // the register tile of a 16-lane group: rows x streamed vectors

// ---- lanes of a 16-lane group ----
__device__ __forceinline__ int quad_xor1_i(int x) { return __builtin_amdgcn_mov_dpp(x, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ int quad_xor2_i(int x) { return __builtin_amdgcn_mov_dpp(x, 0x4E, 0xF, 0xF, true); }
// lane t ^ 4 inside a row of 16: the lower quad of each pair takes lane + 4 (row_shl:4 into banks 0 and 2), the upper lane - 4
__device__ __forceinline__ int row_xor4_i(int x) {
    int t = __builtin_amdgcn_update_dpp(0, x, 0x104, 0xF, 0x5, false);
    return __builtin_amdgcn_update_dpp(t, x, 0x114, 0xF, 0xA, false);
}
__device__ __forceinline__ int row_xor8_i(int x) { return __builtin_amdgcn_update_dpp(0, x, 0x128, 0xF, 0xF, false); }   // row_ror:8
__device__ __forceinline__ float row_xor4(float v) { return __int_as_float(row_xor4_i(__float_as_int(v))); }
__device__ __forceinline__ float row_xor8(float v) { return __int_as_float(row_xor8_i(__float_as_int(v))); }
__device__ __forceinline__ float quad_pair_lo(float v) {   // quad_perm [0,0,2,2]
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xA0, 0xF, 0xF, true));
}
__device__ __forceinline__ float quad_pair_hi(float v) {   // quad_perm [1,1,3,3]
    return __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0xF5, 0xF, 0xF, true));
}
template <int S>
__device__ __forceinline__ uint32_t group_xor(uint32_t v) {   // the value of lane t ^ (1 << S)
    return (uint32_t)(S == 0 ? quad_xor1_i((int)v) : S == 1 ? quad_xor2_i((int)v) : S == 2 ? row_xor4_i((int)v) : row_xor8_i((int)v));
}
template <int S>
__device__ __forceinline__ u64 group_xor(u64 v) {
    return ((u64)group_xor<S>((uint32_t)(v >> 32)) << 32) | group_xor<S>((uint32_t)v);
}
template <typename K>
__device__ __forceinline__ K group_min16(K v) {   // the minimum over the 16 lanes of a group, in every one of them
    K o;
    o = group_xor<0>(v); v = o < v ? o : v;
    o = group_xor<1>(v); v = o < v ? o : v;
    o = group_xor<2>(v); v = o < v ? o : v;
    o = group_xor<3>(v); v = o < v ? o : v;
    return v;
}

// wide::f32x8::reduce_add of v[0..8) held as (v[2 p], v[2 p + 1]) by lane p = t & 3 of every quad (device_util.hpp hreduce8 is the
// one-lane form): MODE 0 = SSE2 build order, 1 = AVX order, 2 = two sequential 4-lane sums
template <int MODE>
__device__ __forceinline__ float hreduce_pairs(f32x2 v) {
    if (MODE == 2) {
        const float e0x = quad_pair_lo(v.x), e0y = quad_pair_lo(v.y), e1x = quad_pair_hi(v.x), e1y = quad_pair_hi(v.y);
        const float w = ((e0x + e0y) + e1x) + e1y;   // lanes 0,1: ((v0+v1)+v2)+v3   lanes 2,3: ((v4+v5)+v6)+v7
        return w + quad_xor2(w);
    }
    if (MODE == 1) {
        const float ux = v.x + quad_xor2(v.x), uy = v.y + quad_xor2(v.y);   // lane 0: v0+v4, v1+v5   lane 1: v2+v6, v3+v7
        const float lo = ux + quad_xor1(ux), hi = uy + quad_xor1(uy);       // (v0+v4)+(v2+v6), (v1+v5)+(v3+v7)
        return lo + hi;
    }
    const float ux = v.x + quad_xor1(v.x), uy = v.y + quad_xor1(v.y);       // lanes 0,1: v0+v2, v1+v3   lanes 2,3: v4+v6, v5+v7
    const float w = ux + uy;
    return w + quad_xor2(w);
}

// ---- the running lists of a group's kTR rows ----
// Slot (t + 16 i) of row r lives in slot[r][i] of lane t, as whatever the kernel stores (type K).  The policy P turns it into the
// integer key it competes with — P::key(stored, slot index), greater is better, slots that do not exist answer the greatest key
// and are never replaced — and a least key into the float that screens candidates, P::screen(key).  thr[r] = the least key.
template <typename K, typename P>
struct GroupLists {
    K slot[kTR][4];
    K thr[kTR];
    float thrf[kTR];

    template <int R>
    __device__ __forceinline__ void threshold(const P& p, int t) {
        K v = p.key(slot[R][0], t);
#pragma unroll
        for (int i = 1; i < 4; ++i) {
            const K k = p.key(slot[R][i], t + 16 * i);
            v = k < v ? k : v;
        }
        v = group_min16(v);
        thr[R] = v;
        thrf[R] = p.screen(v);
    }
    // `stored` (its key beats thr[R]) replaces the first slot that holds the least key
    template <int R>
    __device__ __forceinline__ void insert(const P& p, K stored, int lane, int t) {
        bool done = false;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const u64 b = __ballot(!done && p.key(slot[R][i], t + 16 * i) == thr[R]);
            const uint32_t mine = (uint32_t)(b >> (lane & 48)) & 0xffffu;   // this group's 16 lanes
            if (!done && mine) {
                if (t == __ffs((int)mine) - 1) slot[R][i] = stored;
                done = true;
            }
        }
        threshold<R>(p, t);
    }
    __device__ __forceinline__ void threshold_all(const P& p, int t) {
        threshold<0>(p, t);
        threshold<1>(p, t);
        threshold<2>(p, t);
        threshold<3>(p, t);
    }
    __device__ __forceinline__ void insert_row(int r, const P& p, K stored, int lane, int t) {   // r: a constant after unrolling
        if (r == 0) insert<0>(p, stored, lane, t);
        if (r == 1) insert<1>(p, stored, lane, t);
        if (r == 2) insert<2>(p, stored, lane, t);
        if (r == 3) insert<3>(p, stored, lane, t);
    }
};

// ---- the row tile ----
// Slab rows [tile_row0, tile_row0 + rows_wg) widened to f32 (exact for f16) into xs[rows_wg][xstride]; rows from row_end on are
// zeros.  Loads are clamped to the last row instead of predicated, and four are in flight per thread: a predicated scalar loop paid
// one memory latency per element (150 ms of a 10M-row hubness table).  The caller's next barrier publishes the tile.
__device__ __forceinline__ void load_row_tile(float* xs, const void* slab_base, uint32_t row_stride, bool f32, int dim, uint32_t tile_row0,
                                              uint32_t row_end, int rows_wg, int xstride, int tid, int nthreads) {
    const unsigned char* slab = reinterpret_cast<const unsigned char*>(slab_base);
    const bool vec = (row_stride & 15u) == 0 && (dim & 7) == 0 && (reinterpret_cast<uintptr_t>(slab_base) & 15u) == 0;
    if (vec) {
        const int cpr = dim >> 3, nchunks = rows_wg * cpr;   // 8-element chunks: 16 bytes of f16, 32 of f32
        for (int base = 0; base < nchunks; base += 4 * nthreads) {
            u32x4 lo[4], hi[4];
            int at[4];   // where the chunk goes: -1 = nowhere, < -1 = zeros at -(at + 2)
#pragma unroll
            for (int u = 0; u < 4; ++u) {
                const int idx = base + tid + u * nthreads;
                const int idc = idx < nchunks ? idx : 0;
                const int r = idc / cpr, c = idc - r * cpr;
                const uint32_t row = tile_row0 + (uint32_t)r;
                const unsigned char* p = slab + (size_t)(row < row_end ? row : row_end - 1) * row_stride;
                at[u] = idx < nchunks ? (row < row_end ? r * xstride + 8 * c : -(r * xstride + 8 * c) - 2) : -1;
                if (f32) {
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
                } else if (f32) {
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
            const unsigned char* p = slab + (size_t)(row < row_end ? row : row_end - 1) * row_stride;
            const float v = f32 ? reinterpret_cast<const float*>(p)[e] : (float)reinterpret_cast<const _Float16*>(p)[e];
            xs[r * xstride + e] = row < row_end ? v : 0.0f;
        }
    }
}

// ---- the stream ----
// src[nq][dim] past the group's rows xr (the group's first row + 2 t) in chunks of kQC through qs[kQC][qstride]; per tile of kTQ
// vectors the whole groups of 32 elements are accumulated and finish(acc, xr, qt, index of the tile's first vector) does the rest.
// DIM > 0: compile-time dimension (a multiple of 32), 256 threads, the next chunk prefetched into registers during the arithmetic.
// DIM == 0: any dimension.
template <int DIM, typename Finish>
__device__ __forceinline__ void stream_chunks(const float* src, uint32_t nq, int dim, const float* xr, float* qs, int xstride, int qstride,
                                              int tid, int nthreads, int t, Finish&& finish) {
    constexpr int NPF = DIM ? kQC * DIM / 256 : 1;
    float pf[NPF];
    const size_t q_total = (size_t)nq * dim;
    if (DIM) {   // (loads past the block's end are clamped, not predicated; the store below zeroes them)
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const size_t o = (size_t)(tid + 256 * i);
            pf[i] = src[o < q_total ? o : q_total - 1];
        }
    }
    const int groups = dim >> 5;
    for (uint32_t q0 = 0; q0 < nq; q0 += kQC) {
        __syncthreads();   // the previous chunk has been read by every group
        if (DIM) {
#pragma unroll
            for (int i = 0; i < NPF; ++i) qs[tid + 256 * i] = (size_t)q0 * dim + (size_t)(tid + 256 * i) < q_total ? pf[i] : 0.0f;
        } else {
            for (int idx = tid; idx < kQC * dim; idx += nthreads) {
                const int j = idx / dim, e = idx - j * dim;
                qs[j * qstride + e] = q0 + (uint32_t)j < nq ? src[(size_t)(q0 + j) * dim + e] : 0.0f;
            }
        }
        __syncthreads();
        if (DIM) {
            const size_t base = (size_t)(q0 + kQC) * dim;
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const size_t o = base + (size_t)(tid + 256 * i);
                pf[i] = src[o < q_total ? o : q_total - 1];
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
            for (int g = 0; g < groups; ++g) {
                f32x2 x[kTR], q[kTQ];
#pragma unroll
                for (int r = 0; r < kTR; ++r) x[r] = *reinterpret_cast<const f32x2*>(xr + r * xstride + 32 * g);
#pragma unroll
                for (int j = 0; j < kTQ; ++j) q[j] = *reinterpret_cast<const f32x2*>(qt + j * qstride + 32 * g + 2 * t);
#pragma unroll
                for (int r = 0; r < kTR; ++r)
#pragma unroll
                    for (int j = 0; j < kTQ; ++j) {
                        const f32x2 p = x[r] * q[j];   // a multiply and an add, never an fma (simd.rs:171-186)
                        acc[r][j] = acc[r][j] + p;
                    }
            }
            finish(acc, xr, qt, q0 + (uint32_t)jt);
        }
    }
}

// ---- the finish of a tile: acc -> the kTR x kTQ scores s, in the order of the dot (the table above) ----
// Every phase keeps the tile's (r, j) loops innermost and fully unrolled, so that the accumulators stay in registers.  DIM > 0 has
// neither leftover chunks nor a tail.  The fused tail exists only where FUSED_TAIL is instantiated: hubness's code object must not
// hold a fused operation.
template <int DIM, int MODE, bool LEFTOVERS_BEFORE_TREE, bool FUSED_TAIL>
__device__ __forceinline__ void finish_tile(f32x2 (&acc)[kTR][kTQ], float (&s)[kTR][kTQ], const float* xr, const float* qt, int dim, int xstride,
                                            int qstride, int t) {
    const int chunks = dim >> 3;
    auto leftovers = [&]() {   // lane p = t & 3 of a quad takes elements 2 p and 2 p + 1 of the chunk (xr holds + 2 t)
        const int p2 = 2 * (t & 3);
        for (int c = chunks & ~3; c < chunks; ++c) {
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
    };
    if (DIM == 0 && LEFTOVERS_BEFORE_TREE) {
        if (t < 4) leftovers();   // into accumulator 0, the group's first quad (simd.rs:419-431)
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
    if (DIM == 0 && !LEFTOVERS_BEFORE_TREE) leftovers();   // to the tree's sum, in every quad (simd.rs:192-203, 660-672)
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int j = 0; j < kTQ; ++j) s[r][j] = hreduce_pairs<MODE>(acc[r][j]);
    if (DIM == 0) {
        for (int i = chunks * 8; i < dim; ++i) {   // the tail (simd.rs:214-220 unfused; fused in both byte dots)
            float x[kTR], q[kTQ];
#pragma unroll
            for (int r = 0; r < kTR; ++r) x[r] = xr[r * xstride - 2 * t + i];
#pragma unroll
            for (int j = 0; j < kTQ; ++j) q[j] = qt[j * qstride + i];
#pragma unroll
            for (int r = 0; r < kTR; ++r)
#pragma unroll
                for (int j = 0; j < kTQ; ++j) {
                    if constexpr (FUSED_TAIL) {
                        s[r][j] = __builtin_fmaf(x[r], q[j], s[r][j]);
                    } else {
                        const float p = x[r] * q[j];
                        s[r][j] = s[r][j] + p;
                    }
                }
        }
    }
}

// ---- the host's side ----
// Row stride in LDS: = 8 (mod 16) floats, so that the two groups of a half-wave (rows 4 apart) read disjoint halves of the 64
// banks with ds_read_b64; the streamed vectors are a broadcast.  Four waves, halved until rows, chunk and extra_per_wave bytes fit
// the budget; `fixed`: the compile-time dimension applies (dim is one of fixed_dims and the workgroup kept its four waves).
struct JoinTilePlan {
    int waves, xstride, qstride;
    size_t lds;   // dynamic LDS in bytes; 0 = even one wave does not fit
    bool fixed;
};
inline JoinTilePlan plan_join_tile(uint32_t dim, size_t extra_per_wave, size_t budget, std::initializer_list<uint32_t> fixed_dims) {
    JoinTilePlan p{4, (int)((dim + 15u) & ~15u) + 8, (int)((dim + 1u) & ~1u), 0, false};
    for (uint32_t d : fixed_dims) p.fixed |= d == dim;
    if (p.fixed) p.qstride = (int)dim;
    auto lds_of = [&](int waves) { return ((size_t)waves * kJoinTileRowsPerWave * p.xstride + (size_t)kJoinTileChunk * p.qstride) * 4 + waves * extra_per_wave; };
    while (p.waves > 1 && lds_of(p.waves) > budget) p.waves >>= 1;
    p.lds = lds_of(p.waves) > budget ? 0 : lds_of(p.waves);
    p.fixed = p.fixed && p.waves == 4;
    return p;
}
// kern(args, xstride, qstride) over args.nrows rows, one workgroup per 16 rows of every wave
template <typename Args>
hipError_t launch_join_tile(void (*kern)(Args, int, int), const Args& a, const JoinTilePlan& p, hipStream_t stream) {
    if (p.lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)p.lds);
        if (e != hipSuccess) return e;
    }
    const uint32_t rows_wg = (uint32_t)p.waves * kJoinTileRowsPerWave;
    hipLaunchKernelGGL(kern, dim3((a.nrows + rows_wg - 1) / rows_wg), dim3(p.waves * 64), p.lds, stream, a, p.xstride, p.qstride);
    return hipGetLastError();
}

}  // namespace fsgpu

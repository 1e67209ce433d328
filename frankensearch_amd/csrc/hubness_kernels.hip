// hubness_kernels.hip — the query-hubness table r_d of every slab row (crates/frankensearch-fusion/src/hubness.rs:109-138): the mean
// of the row's k greatest similarities to a background query sample.  A transposed scan: per ROW a top-k over QUERIES.
//
// sim(row, j) = dot_product_f32_f32 (crates/frankensearch-index/src/simd.rs:134-222): four 8-lane accumulators over groups of 32
// (accumulator a, lane l takes element 32 g + 8 a + l; a separate multiply and add — this file is compiled with -ffp-contract=off),
// (acc0 + acc1) + (acc2 + acc3), the leftover 8-element chunks added to that sum AFTER the tree, reduce_add in the index's
// horizontal order, then the last dim % 8 elements as an UNFUSED multiply and add (f32_kernels.hip, the F32-slab byte dot, fuses
// its tail; the f16 byte dot also puts the leftovers into acc0 before the tree).
//
// Mapping.  A dot is 32 independent chains (chain c = 8 a + l holds elements c, 32 + c, 64 + c, ...), each sequential over the
// groups, followed by a fixed tree — so lanes that own chains need no reassociation.  Sixteen lanes form a group; lane t owns the
// ADJACENT chains 2 t and 2 t + 1 (a = t >> 2, l = 2 (t & 3) and + 1), i.e. one 8-byte LDS read per operand and group, and the
// packed f32 multiply / add work on natural register pairs.  A group keeps a register tile of 4 rows x 8 queries (64 accumulators
// per lane; 12 ds_read_b64 per 64 packed multiply-adds).  The tree is two DPP steps inside the 16-lane row (t ^ 4: acc0 + acc1 and
// acc2 + acc3; t ^ 8: their sum), the horizontal add two or three quad steps; every lane of the group ends with the same bits.
//
// A workgroup of W waves owns 16 W rows (4 per group), widened to f32 in LDS once, and streams the whole query sample past them
// in chunks of 16 queries, in the same order in every workgroup (the sample is served from L2 / the Infinity Cache).  Each row's
// running top-k lives in the registers of its group (k <= 64 = 16 lanes x 4 slots) as total_cmp keys; a similarity is inserted
// only when it beats the row's current k-th (a float pre-check, then the exact key compare), replacing the minimum, and the new
// minimum is a 16-lane DPP reduction.  At the end the k keys are rank-sorted through LDS and summed in the canonical order.
#include "kernels.hpp"
#include "device_util.hpp"

namespace fsgpu {

namespace {

typedef float f32x2 __attribute__((ext_vector_type(2)));

constexpr int kQC = (int)kHubQueryChunk;   // queries per LDS chunk
constexpr int kTR = 4, kTQ = 8;            // the register tile of a 16-lane group: rows x queries
constexpr int kHubGroupScratch = kTR * 64 + 64;   // u32 of LDS per group for the final sort

__device__ __forceinline__ uint32_t hub_key(float x) {   // f32::total_cmp as an unsigned key (hubness.rs:135); NaNs keep their place
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float hub_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

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
__device__ __forceinline__ uint32_t group_min16(uint32_t m) {
    uint32_t o;
    o = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0xB1, 0xF, 0xF, true); m = o < m ? o : m;
    o = (uint32_t)__builtin_amdgcn_mov_dpp((int)m, 0x4E, 0xF, 0xF, true); m = o < m ? o : m;
    o = (uint32_t)row_xor4_i((int)m); m = o < m ? o : m;
    o = (uint32_t)row_xor8_i((int)m); m = o < m ? o : m;
    return m;
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

// The running top-k of the group's kTR rows: slot (t + 16 i) of row r in slot[r][i]; slots >= k hold 0xffffffff and never become
// the minimum unless every real slot holds that key too.  thr[r] = the minimum over the row's slots (0 until k real values came).
struct GroupTopK {
    uint32_t slot[kTR][4];
    uint32_t thr[kTR];
    float thrf[kTR];
};

template <int R>
__device__ __forceinline__ void hub_insert(GroupTopK& tk, uint32_t key, int lane, int t) {
    bool done = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const u64 b = __ballot(!done && tk.slot[R][i] == tk.thr[R]);
        const uint32_t mine = (uint32_t)(b >> (lane & 48)) & 0xffffu;   // this group's 16 lanes
        if (!done && mine) {
            if (t == __ffs((int)mine) - 1) tk.slot[R][i] = key;
            done = true;
        }
    }
    uint32_t m = tk.slot[R][0];
#pragma unroll
    for (int i = 1; i < 4; ++i) m = tk.slot[R][i] < m ? tk.slot[R][i] : m;
    m = group_min16(m);
    tk.thr[R] = m;
    tk.thrf[R] = hub_value(m);
}

// tree + leftovers + horizontal add + tail of the tile, then the threshold-gated inserts
template <int DIM, int MODE>
__device__ __forceinline__ void hub_finish_tile(f32x2 (&acc)[kTR][kTQ], GroupTopK& tk, const float* xr, const float* qt, int dim, int xstride,
                                                int qstride, uint32_t q_first, uint32_t nq, int lane, int t) {
    const int chunks = dim >> 3, groups = chunks >> 2;
    const int p2 = 2 * (t & 3);
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
#pragma unroll
        for (int j = 0; j < kTQ; ++j) {
            f32x2 u = acc[r][j];
            u.x = u.x + row_xor4(u.x);   // acc0 + acc1 | acc2 + acc3
            u.y = u.y + row_xor4(u.y);
            u.x = u.x + row_xor8(u.x);   // (acc0 + acc1) + (acc2 + acc3)
            u.y = u.y + row_xor8(u.y);
            if (DIM == 0) {
                for (int c = 4 * groups; c < chunks; ++c) {   // leftover chunks join AFTER the tree (simd.rs:192-203)
                    const f32x2 x = *reinterpret_cast<const f32x2*>(xr + r * xstride - 2 * t + 8 * c + p2);
                    const f32x2 q = *reinterpret_cast<const f32x2*>(qt + j * qstride + 8 * c + p2);
                    const f32x2 p = x * q;
                    u = u + p;
                }
            }
            float s = hreduce_pairs<MODE>(u);
            if (DIM == 0) {
                for (int i = chunks * 8; i < dim; ++i) {   // unfused tail (simd.rs:214-220)
                    const float p = xr[r * xstride - 2 * t + i] * qt[j * qstride + i];
                    s = s + p;
                }
            }
            // a query past the sample's end is not a candidate; the float compare only screens (NaN on either side passes)
            if (q_first + (uint32_t)j < nq && !(s < tk.thrf[r])) {
                const uint32_t key = hub_key(s);
                if (key > tk.thr[r]) {
                    if (r == 0) hub_insert<0>(tk, key, lane, t);
                    if (r == 1) hub_insert<1>(tk, key, lane, t);
                    if (r == 2) hub_insert<2>(tk, key, lane, t);
                    if (r == 3) hub_insert<3>(tk, key, lane, t);
                }
            }
        }
    }
}

// DIM > 0: compile-time dimension (a multiple of 32), 256 threads, the next query chunk prefetched into registers during the
// arithmetic.  DIM == 0: any dimension up to kHubMaxDim, 64 / 128 / 256 threads by what fits the LDS.
template <int DIM, int MODE>
__global__ __launch_bounds__(256) void hubness_kernel(HubnessArgs a, int xstride, int qstride) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int dim = DIM ? DIM : (int)a.dim;
    const int nthreads = (int)blockDim.x, rows_wg = (nthreads >> 6) * (int)kHubRowsPerWave;
    float* xs = reinterpret_cast<float*>(smem);                                   // [rows_wg][xstride]
    float* qs = xs + (size_t)rows_wg * xstride;                                   // [kQC][qstride]
    uint32_t* gs = reinterpret_cast<uint32_t*>(qs + (size_t)kQC * qstride);       // [groups][kHubGroupScratch]: the final sort
    const int tid = (int)threadIdx.x, lane = tid & 63, t = lane & 15;
    const int gid = tid >> 4;   // group of the workgroup
    const uint32_t tile_row0 = a.row0 + blockIdx.x * (uint32_t)rows_wg, row_end = a.row0 + a.nrows;
    const uint32_t nq = a.nq;
    const int k = (int)a.k;

    // the tile's rows, widened to f32 (exact for f16); rows past the end are zeros and are never written out.  Loads are clamped to
    // the last row instead of predicated, and four are in flight per thread: a predicated scalar loop paid one memory latency per
    // element (150 ms of a 10M-row table).
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
                if (a.slab_f32) {
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
                } else if (a.slab_f32) {
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
            const float v = a.slab_f32 ? reinterpret_cast<const float*>(p)[e] : (float)reinterpret_cast<const _Float16*>(p)[e];
            xs[r * xstride + e] = row < row_end ? v : 0.0f;
        }
    }

    GroupTopK tk;
#pragma unroll
    for (int r = 0; r < kTR; ++r) {
#pragma unroll
        for (int i = 0; i < 4; ++i) tk.slot[r][i] = (t + 16 * i < k) ? 0u : 0xffffffffu;
        tk.thr[r] = 0u;
        tk.thrf[r] = hub_value(0u);   // a NaN: everything passes the screen until k values are held
    }

    constexpr int NPF = DIM ? kQC * DIM / 256 : 1;
    float pf[NPF];
    const size_t q_total = (size_t)nq * dim;
    if (DIM) {   // (loads past the sample's end are clamped, not predicated; the store below zeroes them)
#pragma unroll
        for (int i = 0; i < NPF; ++i) {
            const size_t o = (size_t)(tid + 256 * i);
            pf[i] = a.queries[o < q_total ? o : q_total - 1];
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
                qs[j * qstride + e] = q0 + (uint32_t)j < nq ? a.queries[(size_t)(q0 + j) * dim + e] : 0.0f;
            }
        }
        __syncthreads();
        if (DIM) {
            const size_t base = (size_t)(q0 + kQC) * dim;
#pragma unroll
            for (int i = 0; i < NPF; ++i) {
                const size_t o = base + (size_t)(tid + 256 * i);
                pf[i] = a.queries[o < q_total ? o : q_total - 1];
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
            hub_finish_tile<DIM, MODE>(acc, tk, xr, qt, dim, xstride, qstride, q0 + (uint32_t)jt, nq, lane, t);
        }
    }

    // per row: the k keys through LDS, rank-sorted (greatest first; equal keys by slot), then the canonical sum
    uint32_t* g = gs + gid * kHubGroupScratch;   // [kTR][64] keys | [64] sorted
    wave_lds_fence();
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) g[r * 64 + t + 16 * i] = tk.slot[r][i];
    wave_lds_fence();
    uint32_t* sorted = g + kTR * 64;
#pragma unroll 1
    for (int r = 0; r < kTR; ++r) {
        const uint32_t* keys = g + r * 64;
        uint32_t mine[4];
        int rank[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < 4; ++i) mine[i] = keys[t + 16 * i];
#pragma unroll 1
        for (int s = 0; s < k; ++s) {
            const uint32_t other = keys[s];
#pragma unroll
            for (int i = 0; i < 4; ++i) rank[i] += (other > mine[i] || (other == mine[i] && s < t + 16 * i)) ? 1 : 0;
        }
        wave_lds_fence();   // the previous row's sorted keys have been read
#pragma unroll
        for (int i = 0; i < 4; ++i)
            if (t + 16 * i < k) sorted[rank[i]] = mine[i];
        wave_lds_fence();
        const uint32_t row = tile_row0 + (uint32_t)(gid * kTR + r);
        if (row < row_end) {
            // v_1 >= ... >= v_k; s = v_1; s += v_2 .. v_{k-1}; v_k + s — one of the orders hubness.rs:136-137 can produce.  The
            // division by k is hubness_divide_kernel's: its expansion is made of fused operations, which this kernel's ISA must
            // not contain (tests/test_hubness_contract.py reads it).
            float s = hub_value(sorted[0]);
#pragma unroll 1
            for (int i = 1; i + 1 < k; ++i) s = s + hub_value(sorted[i]);
            if (t == 0) a.out[row] = k == 1 ? s : hub_value(sorted[k - 1]) + s;
            if (a.out_topk) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (t + 16 * i < k) a.out_topk[(size_t)row * k + (t + 16 * i)] = hub_value(sorted[t + 16 * i]);
            }
        }
    }
}

// out[i] = out[i] / (float)k over rows [row0, row0 + n): `sum / k as f32` (hubness.rs:137), correctly rounded
__global__ __launch_bounds__(256) void hubness_divide_kernel(float* out, uint32_t row0, uint32_t n, float k) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) out[row0 + i] = out[row0 + i] / k;
}

template <int DIM, int MODE>
hipError_t launch_t(const HubnessArgs& a, int waves, int xstride, int qstride, size_t lds, hipStream_t stream) {
    auto kern = hubness_kernel<DIM, MODE>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    const uint32_t rows_wg = (uint32_t)waves * kHubRowsPerWave;
    const uint32_t grid = (a.nrows + rows_wg - 1) / rows_wg;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(waves * 64), lds, stream, a, xstride, qstride);
    hipLaunchKernelGGL(hubness_divide_kernel, dim3((a.nrows + 255) / 256), dim3(256), 0, stream, a.out, a.row0, a.nrows, (float)a.k);
    return hipGetLastError();
}

template <int DIM>
hipError_t launch_m(const HubnessArgs& a, int waves, int xstride, int qstride, size_t lds, hipStream_t stream) {
    if (a.hreduce == 2) return launch_t<DIM, 2>(a, waves, xstride, qstride, lds, stream);
    if (a.hreduce == 1) return launch_t<DIM, 1>(a, waves, xstride, qstride, lds, stream);
    return launch_t<DIM, 0>(a, waves, xstride, qstride, lds, stream);
}

}  // namespace

// rows [row0, row0 + nrows) of the slab against the whole sample; 1 <= k <= kHubMaxK, 1 <= dim <= kHubMaxDim, nq >= 1
hipError_t launch_hubness(const HubnessArgs& a, hipStream_t stream) {
    if (a.nrows == 0) return hipSuccess;
    if (a.k < 1 || a.k > kHubMaxK || a.dim < 1 || a.dim > kHubMaxDim || a.nq < 1 || a.k > a.nq) return hipErrorInvalidValue;
    // row stride in LDS: = 8 (mod 16) floats, so that the two groups of a half-wave (rows 4 apart) read disjoint halves of the
    // 64 banks with ds_read_b64; the queries are a broadcast
    const int xstride = (int)((a.dim + 15u) & ~15u) + 8;
    const bool fixed = a.dim == 384 || a.dim == 256;
    const int qstride = fixed ? (int)a.dim : (int)((a.dim + 1u) & ~1u);
    auto lds_of = [&](int waves) {
        return ((size_t)waves * kHubRowsPerWave * xstride + (size_t)kHubQueryChunk * qstride + (size_t)waves * 4 * kHubGroupScratch) * 4;
    };
    int waves = 4;
    while (waves > 1 && lds_of(waves) > kHubLdsBudget) waves >>= 1;
    const size_t lds = lds_of(waves);
    if (lds > kHubLdsBudget) return hipErrorInvalidValue;
    if (fixed && waves == 4) return a.dim == 384 ? launch_m<384>(a, 4, xstride, qstride, lds, stream) : launch_m<256>(a, 4, xstride, qstride, lds, stream);
    return launch_m<0>(a, waves, xstride, qstride, lds, stream);
}

}  // namespace fsgpu

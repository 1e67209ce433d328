// hubness_kernels.hip — the query-hubness table r_d of every slab row (crates/frankensearch-fusion/src/hubness.rs:109-138): the mean
// of the row's k greatest similarities to a background query sample.  A transposed scan: per ROW a top-k over QUERIES, on
// join_tile.hpp's tile (the mapping of lanes to the dot's chains is described there).
//
// sim(row, j) = dot_product_f32_f32 (crates/frankensearch-index/src/simd.rs:134-222): leftover chunks after the tree, an UNFUSED
// tail.  This file's code object holds no fused operation at all (tests/test_hubness_contract.py reads it), hence the division in
// a kernel of its own.
//
// Each row's running top-k (k <= 64) holds f32::total_cmp keys; slots >= k hold 0xffffffff from the start and never become the
// minimum unless every real slot holds that key too, the real ones start at 0, below every similarity.  At the end the k keys are
// rank-sorted through LDS and summed in the canonical order.
#include "join_tile.hpp"

namespace fsgpu {

namespace {

constexpr int kHubGroupScratch = kTR * 64 + 64;   // u32 of LDS per group for the final sort

__device__ __forceinline__ uint32_t hub_key(float x) {   // f32::total_cmp as an unsigned key (hubness.rs:135); NaNs keep their place
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
__device__ __forceinline__ float hub_value(uint32_t key) {
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7fffffffu) : ~key);
}

struct HubSlots {   // the stored word is the key; the screen of the initial threshold 0 is a NaN, which lets everything pass
    __device__ __forceinline__ uint32_t key(uint32_t stored, int) const { return stored; }
    __device__ __forceinline__ float screen(uint32_t key) const { return hub_value(key); }
};

// DIM > 0: 256 threads; DIM == 0: any dimension up to kHubMaxDim, 64 / 128 / 256 threads by what fits the LDS
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

    load_row_tile(xs, a.slab, a.row_stride, a.slab_f32 != 0, dim, tile_row0, row_end, rows_wg, xstride, tid, nthreads);

    const HubSlots pol;
    GroupLists<uint32_t, HubSlots> tk;
#pragma unroll
    for (int r = 0; r < kTR; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) tk.slot[r][i] = (t + 16 * i < k) ? 0u : 0xffffffffu;
    tk.threshold_all(pol, t);

    const float* xr0 = xs + (size_t)(gid * kTR) * xstride + 2 * t;
    stream_chunks<DIM>(a.queries, nq, dim, xr0, qs, xstride, qstride, tid, nthreads, t,
                       [&](f32x2(&acc)[kTR][kTQ], const float* xr, const float* qt, uint32_t q_first) {
        float s[kTR][kTQ];
        finish_tile<DIM, MODE, false, false>(acc, s, xr, qt, dim, xstride, qstride, t);
#pragma unroll
        for (int r = 0; r < kTR; ++r)
#pragma unroll
            for (int j = 0; j < kTQ; ++j) {
                // a query past the sample's end is not a candidate; the float compare only screens (NaN on either side passes)
                if (q_first + (uint32_t)j < nq && !(s[r][j] < tk.thrf[r])) {
                    const uint32_t key = hub_key(s[r][j]);
                    if (key > tk.thr[r]) tk.insert_row(r, pol, key, lane, t);
                }
            }
    });

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
hipError_t launch_t(const HubnessArgs& a, const JoinTilePlan& p, hipStream_t stream) {
    hipError_t e = launch_join_tile(hubness_kernel<DIM, MODE>, a, p, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hubness_divide_kernel, dim3((a.nrows + 255) / 256), dim3(256), 0, stream, a.out, a.row0, a.nrows, (float)a.k);
    return hipGetLastError();
}

template <int DIM>
hipError_t launch_m(const HubnessArgs& a, const JoinTilePlan& p, hipStream_t stream) {
    if (a.hreduce == 2) return launch_t<DIM, 2>(a, p, stream);
    if (a.hreduce == 1) return launch_t<DIM, 1>(a, p, stream);
    return launch_t<DIM, 0>(a, p, stream);
}

}  // namespace

// rows [row0, row0 + nrows) of the slab against the whole sample; 1 <= k <= kHubMaxK, 1 <= dim <= kHubMaxDim, nq >= 1
hipError_t launch_hubness(const HubnessArgs& a, hipStream_t stream) {
    if (a.nrows == 0) return hipSuccess;
    if (a.k < 1 || a.k > kHubMaxK || a.dim < 1 || a.dim > kHubMaxDim || a.nq < 1 || a.k > a.nq) return hipErrorInvalidValue;
    const JoinTilePlan p = plan_join_tile(a.dim, 4 * kHubGroupScratch * sizeof(uint32_t), kHubLdsBudget, {384, 256});
    if (p.lds == 0) return hipErrorInvalidValue;
    if (p.fixed) return a.dim == 384 ? launch_m<384>(a, p, stream) : launch_m<256>(a, p, stream);
    return launch_m<0>(a, p, stream);
}

}  // namespace fsgpu

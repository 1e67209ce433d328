// scan_common.hpp — device helpers shared by the scan kernels (scan_kernels.hip, scan_mq_kernel.hip).
#pragma once

#include "device_util.hpp"
#include "kernels.hpp"

namespace fsgpu {
namespace scan_detail {

constexpr int kWavesPerBlock = 4;
constexpr int kRowsPerTile = 16;

__device__ __forceinline__ u32x4 load_nt16(const u32x4* p) { return __builtin_nontemporal_load(p); }

// ---- per-wave top-k state over an LDS buffer of CAP packed entries ---------------------------------
template <int CAP>
struct WaveTopK {
    u64* buf;   // CAP entries (LDS)
    int count;  // wave-uniform
    __device__ __forceinline__ void init(u64* b) {
        buf = b;
        count = 0;
    }
    // Sort, trim to k, return the new threshold sortkey (0 while fewer than k entries are held).
    __device__ __forceinline__ u64 compact(int k, int lane) {
        for (int i = count + lane; i < CAP; i += 64) buf[i] = kEmpty;
        wave_sort_desc<CAP>(buf, lane);
        if (count > k) count = k;
        u64 thr = 0;
        if (count == k) thr = sortkey(buf[k - 1]);
        return thr;
    }
};

// One chunk (8 f16 x 8 f32) into the lane's 8 accumulators: separate multiply and add.
__device__ __forceinline__ void chunk_mac(float (&acc)[8], const u32x4& w, const float4& q0, const float4& q1) {
    const half8 h = __builtin_bit_cast(half8, w);
    float p;
    p = (float)h[0] * q0.x; acc[0] = acc[0] + p;
    p = (float)h[1] * q0.y; acc[1] = acc[1] + p;
    p = (float)h[2] * q0.z; acc[2] = acc[2] + p;
    p = (float)h[3] * q0.w; acc[3] = acc[3] + p;
    p = (float)h[4] * q1.x; acc[4] = acc[4] + p;
    p = (float)h[5] * q1.y; acc[5] = acc[5] + p;
    p = (float)h[6] * q1.z; acc[6] = acc[6] + p;
    p = (float)h[7] * q1.w; acc[7] = acc[7] + p;
}

// (s0+s1)+(s2+s3) across the quad, then the horizontal add; every lane of the quad gets the result.
__device__ __forceinline__ float quad_finish(const float (&acc)[8], int hreduce) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float u = acc[j] + quad_xor1(acc[j]);  // lanes 0,1: s0+s1   lanes 2,3: s2+s3
        v[j] = u + quad_xor2(u);                     // (s0+s1)+(s2+s3)
    }
    return hreduce8(v, hreduce);
}

// ---- dot_product_f32_bytes_f32 (simd.rs:581-702): its operation order for one row on a quad of lanes ---------------------------
// Lane a owns accumulator a: elements [32 g + 8 a, 32 g + 8 a + 8) of every group of 32.  Used by dot_rows_f32_kernel
// (f32_kernels.hip) and by the F32-row re-score of the selections (mfma_scan.hip).

// 8 consecutive f32 of a row; vec: the address is 16-byte aligned (two dwordx4 loads)
__device__ __forceinline__ void load_f32x8(float (&x)[8], const float* w, bool vec) {
    if (vec) {
        const float4 lo = *reinterpret_cast<const float4*>(w), hi = *reinterpret_cast<const float4*>(w + 4);
        x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w;
        x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
    } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) x[j] = w[j];
    }
}

// One chunk (8 f32 x 8 f32) into 8 accumulators: separate multiply and add.
__device__ __forceinline__ void chunk_mac_f32(float (&acc)[8], const float (&x)[8], const float* q) {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float p = x[j] * q[j];
        acc[j] = acc[j] + p;
    }
}

// (acc0+acc1)+(acc2+acc3) across the quad, THEN the leftover 8-element chunks (the f16 form adds them to acc0 before the combine),
// the horizontal add, and a fused multiply-add per element of the last dim % 8.  Leftovers and tail are computed redundantly by
// the quad's lanes, which all end with the same bits.  w = the row, q = the query (dim floats each).
__device__ __forceinline__ float quad_finish_f32(const float (&acc)[8], const float* w, const float* q, int dim, int hreduce) {
    const int chunks = dim >> 3, groups = chunks >> 2;
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const float u = acc[j] + quad_xor1(acc[j]);  // lanes 0,1: acc0+acc1   lanes 2,3: acc2+acc3
        v[j] = u + quad_xor2(u);                     // (acc0+acc1)+(acc2+acc3)
    }
    for (int c = 4 * groups; c < chunks; ++c)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const float p = w[8 * c + j] * q[8 * c + j];
            v[j] = v[j] + p;
        }
    float s = hreduce8(v, hreduce);
    for (int i = chunks * 8; i < dim; ++i) s = __builtin_fmaf(w[i], q[i], s);
    return s;
}

// The whole dot of one row for lane a of its quad; BATCH groups' row loads are in flight at a time.
template <int BATCH>
__device__ __forceinline__ float quad_dot_f32(const float* w, const float* q, int dim, int a, bool vec, int hreduce) {
    const int groups = dim >> 5;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    for (int g0 = 0; g0 < groups; g0 += BATCH) {
        float x[BATCH][8];
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
            if (g0 + b < groups) load_f32x8(x[b], w + 32 * (g0 + b) + 8 * a, vec);
#pragma unroll
        for (int b = 0; b < BATCH; ++b)
            if (g0 + b < groups) chunk_mac_f32(acc, x[b], q + 32 * (g0 + b) + 8 * a);
    }
    return quad_finish_f32(acc, w, q, dim, hreduce);
}


}  // namespace scan_detail
}  // namespace fsgpu

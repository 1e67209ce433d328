// index_build_kernels.hip — the device passes of the index builder (index_builder.cpp).
//
// INGEST, once per add call: one pass over the call's [n, dim] f32 rows that
//   * gives every row the verdict of VectorIndexWriter::write_record (crates/frankensearch-index/src/lib.rs:3635-3673,
//     vector_signal_usable :6133-6142): every element finite, then norm_sq = sum of v * v in ONE f32 accumulator, elements in order,
//     a separate multiply and add (the library is built with -ffp-contract=off), f32 subnormals kept, must be > 0 and finite;
//   * stages the row at its arrival position, encoded for the slab: round-to-nearest-even f16 (v_cvt_f16_f32, as the FSVI writer's
//     encode_rows_f16_kernel; values beyond the f16 range become +-inf as f16::from_f32 makes them) or the raw little-endian f32.
// A wave owns 64 rows.  They reach it through LDS in tiles of 64 columns: the global loads are side by side along the rows (16 bytes
// per lane, 256 contiguous bytes per row and instruction, when the rows allow it; 4 bytes per lane else) and the staged row is written
// from the same registers; then lane r walks row r of the tile from left to right and carries its accumulator from tile to tile.
// The first offending row of the call is an atomicMin on one word; the host decides what the call does with it.
//
// PERMUTE, at finish: staged rows in arrival order -> the slab in (hash, doc id) order, one whole row per slab row through a u32
// permutation.  A sorted-by-hash order has no runs to speak of, so this is a gather of rows and not compact_runs_kernel's segmented
// copy: a wave owns up to 64 consecutive slab rows (about 16 KB), lane r resolves the source address of row r once, and the rows move
// in the widest unit their length allows (16, 8, 4 or 2 bytes), four units per lane in flight.  Every byte offset is 64-bit.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef float bf32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t bu32x4 __attribute__((ext_vector_type(4)));
typedef uint32_t bu32x2 __attribute__((ext_vector_type(2)));

constexpr uint32_t kTileStride = kBuildTileCols + 4;   // floats between the rows of an LDS tile: rows stay 16-byte aligned
constexpr uint32_t kIngestWaves = 2;                   // per workgroup: 2 x 64 x 68 x 4 = 34,816 bytes of LDS

__device__ __forceinline__ unsigned char* staged_row(unsigned char* const* chunks, uint32_t chunk_rows, u64 pos, uint32_t row_bytes) {
    const u64 c = pos / chunk_rows;
    return chunks[c] + (pos - c * chunk_rows) * (u64)row_bytes;
}

__device__ __forceinline__ unsigned short f16_bits(float v) { return __builtin_bit_cast(unsigned short, (_Float16)v); }

template <bool VEC, bool F16>
__global__ __launch_bounds__(kIngestWaves * 64) void build_ingest_kernel(IngestArgs a) {
    __shared__ __attribute__((aligned(16))) float tiles[kIngestWaves][kBuildTileRows * kTileStride];
    __shared__ unsigned char* row_ptr[kIngestWaves][kBuildTileRows];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint32_t row0 = (blockIdx.x * kIngestWaves + w) * kBuildTileRows;
    const uint32_t rows = row0 < a.n ? (a.n - row0 < kBuildTileRows ? a.n - row0 : kBuildTileRows) : 0u;   // of this wave
    constexpr uint32_t kElem = F16 ? 2u : 4u;
    float* tile = tiles[w];
    if (lane < rows) row_ptr[w][lane] = staged_row(a.chunks, a.chunk_rows, a.first_pos + row0 + lane, a.dim * kElem);
    __syncthreads();
    float acc = 0.0f;
    bool nonfinite = false;
    for (uint32_t c0 = 0; c0 < a.dim; c0 += kBuildTileCols) {
        const uint32_t cols = a.dim - c0 < kBuildTileCols ? a.dim - c0 : kBuildTileCols;
        if constexpr (VEC) {
            // 16 lanes along a row, 4 rows per instruction; every load of the tile is issued before the first use
            const uint32_t sub = lane >> 4, cu = (lane & 15u) * 4u;
            bf32x4 v[16];
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t r = sub + 4u * i;
                v[i] = bf32x4{0.f, 0.f, 0.f, 0.f};
                if (r < rows && cu < cols) v[i] = *reinterpret_cast<const bf32x4*>(a.src + (size_t)(row0 + r) * a.dim + c0 + cu);
            }
#pragma unroll
            for (uint32_t i = 0; i < 16; ++i) {
                const uint32_t r = sub + 4u * i;
                if (r < rows && cu < cols) {
                    *reinterpret_cast<bf32x4*>(tile + r * kTileStride + cu) = v[i];
                    unsigned char* d = row_ptr[w][r] + (size_t)(c0 + cu) * kElem;
                    if constexpr (F16) {
                        bu32x2 h;
                        h.x = (uint32_t)f16_bits(v[i].x) | ((uint32_t)f16_bits(v[i].y) << 16);
                        h.y = (uint32_t)f16_bits(v[i].z) | ((uint32_t)f16_bits(v[i].w) << 16);
                        *reinterpret_cast<bu32x2*>(d) = h;
                    } else {
                        *reinterpret_cast<bf32x4*>(d) = v[i];
                    }
                }
            }
        } else {
            // any dimension, any alignment: lane = column, 16 rows per batch
#pragma unroll 1
            for (uint32_t rb = 0; rb < kBuildTileRows; rb += 16) {
                float v[16];
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t r = rb + i;
                    v[i] = 0.f;
                    if (r < rows && lane < cols) v[i] = a.src[(size_t)(row0 + r) * a.dim + c0 + lane];
                }
#pragma unroll
                for (uint32_t i = 0; i < 16; ++i) {
                    const uint32_t r = rb + i;
                    if (r < rows && lane < cols) {
                        tile[r * kTileStride + lane] = v[i];
                        unsigned char* d = row_ptr[w][r] + (size_t)(c0 + lane) * kElem;
                        if constexpr (F16) *reinterpret_cast<unsigned short*>(d) = f16_bits(v[i]);
                        else *reinterpret_cast<float*>(d) = v[i];
                    }
                }
            }
        }
        __syncthreads();
        if (lane < rows) {
            const float* t = tile + lane * kTileStride;
            uint32_t j = 0;
            for (; j + 4 <= cols; j += 4) {
                const bf32x4 q = *reinterpret_cast<const bf32x4*>(t + j);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x = q[e];
                    nonfinite |= (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u;
                    const float p = x * x;
                    acc = acc + p;
                }
            }
            for (; j < cols; ++j) {
                const float x = t[j];
                nonfinite |= (__builtin_bit_cast(uint32_t, x) & 0x7f800000u) == 0x7f800000u;
                const float p = x * x;
                acc = acc + p;
            }
        }
        __syncthreads();
    }
    if (lane < rows) {
        const bool norm_ok = acc > 0.0f && (__builtin_bit_cast(uint32_t, acc) & 0x7f800000u) != 0x7f800000u;
        const uint32_t rule = nonfinite ? kBuildNonFinite : (norm_ok ? 0u : kBuildBadNorm);
        if (rule) atomicMin(a.verdict, ((a.first_row + row0 + lane) << 8) | rule);
    }
}

constexpr uint32_t kPermuteWaves = 4;
constexpr uint32_t kPermuteWaveBytes = 16 * 1024;
constexpr uint32_t kPermuteWaveRows = 64;

template <typename V>
__global__ __launch_bounds__(kPermuteWaves * 64) void build_permute_kernel(PermuteArgs a, uint32_t rows_per_wave) {
    __shared__ const unsigned char* src_ptr[kPermuteWaves][kPermuteWaveRows];
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const u64 r0 = a.row_begin + ((u64)blockIdx.x * kPermuteWaves + w) * rows_per_wave;
    const uint32_t rows = r0 < a.row_end ? (uint32_t)(a.row_end - r0 < rows_per_wave ? a.row_end - r0 : rows_per_wave) : 0u;
    if (lane < rows) src_ptr[w][lane] = staged_row(a.chunks, a.chunk_rows, a.perm[r0 + lane], a.row_bytes);
    __syncthreads();
    if (rows == 0) return;
    const uint32_t upr = a.row_bytes / (uint32_t)sizeof(V);   // units per row
    const uint32_t total = rows * upr;
    unsigned char* out = a.out + r0 * (u64)a.row_bytes;
    for (uint32_t t = lane; t < total; t += 256) {
        V v[4];
        uint32_t rr[4], u[4];
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i) {
            const uint32_t ti = t + 64u * i;
            rr[i] = ti / upr;
            u[i] = ti - rr[i] * upr;
            if (ti < total) v[i] = reinterpret_cast<const V*>(src_ptr[w][rr[i]])[u[i]];
        }
#pragma unroll
        for (uint32_t i = 0; i < 4; ++i)
            if (t + 64u * i < total) reinterpret_cast<V*>(out + (u64)rr[i] * a.row_bytes)[u[i]] = v[i];
    }
}

}  // namespace

// a.n <= kBuildLaunchRows and a.n * a.dim < 2^31 are the caller's to keep (index_builder.cpp slices a call)
hipError_t launch_build_ingest(const IngestArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (!a.src || !a.chunks || !a.verdict) return hipErrorInvalidValue;   // (a builder without a chunk table must not get this far)
    if (a.n > kBuildLaunchRows || (u64)a.n * a.dim >= (1ull << 31) || a.dim == 0 || a.chunk_rows == 0) return hipErrorInvalidValue;
    const unsigned blocks = (a.n + kIngestWaves * kBuildTileRows - 1) / (kIngestWaves * kBuildTileRows);
    // 16-byte loads need 16-byte aligned rows: dim % 4 == 0 and an aligned block (the staging chunks are allocations of their own)
    const bool vec = a.dim % 4 == 0 && (reinterpret_cast<uintptr_t>(a.src) & 15u) == 0;
    const dim3 grid(blocks), block(kIngestWaves * 64);
    if (vec && a.to_f16) hipLaunchKernelGGL((build_ingest_kernel<true, true>), grid, block, 0, stream, a);
    else if (vec) hipLaunchKernelGGL((build_ingest_kernel<true, false>), grid, block, 0, stream, a);
    else if (a.to_f16) hipLaunchKernelGGL((build_ingest_kernel<false, true>), grid, block, 0, stream, a);
    else hipLaunchKernelGGL((build_ingest_kernel<false, false>), grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_build_permute(const PermuteArgs& a, hipStream_t stream) {
    if (a.row_end <= a.row_begin) return hipSuccess;
    if (!a.chunks || !a.perm || !a.out) return hipErrorInvalidValue;
    if (a.row_end - a.row_begin > kBuildLaunchRows || a.row_bytes < 2 || a.row_bytes % 2 || a.chunk_rows == 0) return hipErrorInvalidValue;
    uint32_t rows_per_wave = kPermuteWaveBytes / a.row_bytes;
    rows_per_wave = rows_per_wave < 1 ? 1 : (rows_per_wave > kPermuteWaveRows ? kPermuteWaveRows : rows_per_wave);
    const u64 rows = a.row_end - a.row_begin;
    const u64 waves = (rows + rows_per_wave - 1) / rows_per_wave;
    const dim3 grid((unsigned)((waves + kPermuteWaves - 1) / kPermuteWaves)), block(kPermuteWaves * 64);
    if (a.row_bytes % 16 == 0) hipLaunchKernelGGL(build_permute_kernel<bu32x4>, grid, block, 0, stream, a, rows_per_wave);
    else if (a.row_bytes % 8 == 0) hipLaunchKernelGGL(build_permute_kernel<bu32x2>, grid, block, 0, stream, a, rows_per_wave);
    else if (a.row_bytes % 4 == 0) hipLaunchKernelGGL(build_permute_kernel<uint32_t>, grid, block, 0, stream, a, rows_per_wave);
    else hipLaunchKernelGGL(build_permute_kernel<unsigned short>, grid, block, 0, stream, a, rows_per_wave);
    return hipGetLastError();
}

}  // namespace fsgpu

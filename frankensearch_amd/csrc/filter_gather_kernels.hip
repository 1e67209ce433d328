// filter_gather_kernels.hip — a filter per query in one batched call (gfx950): the resident allow bitmap turned into its ascending
// row list on the device, and a segmented gather scan that scores every selective filter's rows against the queries that name it.
//
// The reference scores only the allowed rows when a filter lets through fewer than 1/50 of the corpus (try_gather_filtered /
// scan_gather_positions, crates/frankensearch-index/src/search.rs:1114-1255).  Here the queries of a call are grouped by filter, and a
// group's rows travel from HBM to the LDS ONCE for all of the group's queries:
//   grid (blocks, groups): block (b, g) walks the 64-row tiles b, b + nblocks_g, ... of group g's row list; a tile's live rows are
//   staged into LDS (rows 64 bytes apart modulo 256, so that the four quads of a ds_read_b128 lane group read four different
//   16-bank windows), then wave w scores the tile against the group's queries w, w + 4, ...: a quad per row, four rows per lane.
// Arithmetic: the dot of gather_dot_kernel / the exact scan (scan_common.hpp: chunk_mac into accumulator c mod 4 with a separate
// multiply and add, leftover chunks into accumulator 0, quad_finish with the index's hreduce order), so the score bits are the exact
// kernels' by construction.  Selection over packed (score bits << 32 | row) entries, per (query, block): for k <= 64 the k best so far
// sit one per lane and a row enters when it beats the worst of them — parked in the block's list between tiles, sorted once behind the
// block's last tile; for k <= 256 WaveTopK over an LDS buffer, the list reloaded per tile to tighten the threshold.  One best-first
// list of k entries per (query, block) goes to merge_topk_kernel (scan_kernels.hip).  Nothing is sized queries x rows.
#pragma clang fp contract(off)

#include "scan_common.hpp"

namespace fsgpu {

using namespace scan_detail;

// ---- bitmap -> ascending row list ---------------------------------------------------------------------------------------------------
// (1) per 64-bit word a popcount and an exclusive scan inside blocks of kRowListWordsPerBlock words, (2) an exclusive scan over the
// blocks' totals, (3) the expand: every word writes the ids of its set bits at its offset.  Bits past nrows in the tail word do not count.

__device__ __forceinline__ u64 row_list_word(const u64* __restrict__ words, uint32_t w, uint32_t nwords, uint32_t nrows) {
    if (w >= nwords) return 0ull;
    u64 v = words[w];
    if (w + 1 == nwords && (nrows & 63u)) v &= (1ull << (nrows & 63u)) - 1ull;
    return v;
}

__global__ __launch_bounds__(256) void filter_row_list_count_kernel(const u64* __restrict__ words, uint32_t nwords, uint32_t nrows,
                                                                    uint32_t* __restrict__ word_off, uint32_t* __restrict__ block_sum) {
    __shared__ uint32_t s_wave[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t w0 = (blockIdx.x * 256u + (uint32_t)tid) * 4u;   // four consecutive words per thread
    uint32_t c[4], sum = 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        c[j] = (uint32_t)__popcll(row_list_word(words, w0 + j, nwords, nrows));
        sum += c[j];
    }
    // inclusive scan of the threads' sums over the wave, then over the four waves
    uint32_t inc = sum;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off);
        if (lane >= off) inc += o;
    }
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t base = 0;
    for (int x = 0; x < wave; ++x) base += s_wave[x];
    uint32_t run = base + inc - sum;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (w0 + j < nwords) word_off[w0 + j] = run;
        run += c[j];
    }
    if (tid == 255) block_sum[blockIdx.x] = base + inc;
}

// one block: block_sum[0 .. nblocks) -> its exclusive scan in place, the total into *total
__global__ __launch_bounds__(256) void filter_row_list_scan_kernel(uint32_t* __restrict__ block_sum, uint32_t nblocks, uint32_t* __restrict__ total) {
    __shared__ uint32_t s_wave[4];
    __shared__ uint32_t s_carry;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_carry = 0;
    __syncthreads();
    for (uint32_t b0 = 0; b0 < nblocks; b0 += 256) {
        const uint32_t i = b0 + (uint32_t)tid;
        const uint32_t v = i < nblocks ? block_sum[i] : 0u;
        uint32_t inc = v;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t o = __shfl_up(inc, off);
            if (lane >= off) inc += o;
        }
        if (lane == 63) s_wave[wave] = inc;
        __syncthreads();
        uint32_t base = s_carry;
        for (int x = 0; x < wave; ++x) base += s_wave[x];
        if (i < nblocks) block_sum[i] = base + inc - v;
        __syncthreads();
        if (tid == 255) s_carry = base + inc;
        __syncthreads();
    }
    if (tid == 0) *total = s_carry;
}

__global__ __launch_bounds__(256) void filter_row_list_expand_kernel(const u64* __restrict__ words, uint32_t nwords, uint32_t nrows,
                                                                     const uint32_t* __restrict__ word_off,
                                                                     const uint32_t* __restrict__ block_off, uint32_t cap,
                                                                     uint32_t* __restrict__ out_rows) {
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= nwords) return;
    u64 v = row_list_word(words, w, nwords, nrows);
    uint32_t at = block_off[w / kRowListWordsPerBlock] + word_off[w];
    while (v) {
        const int b = __builtin_ctzll(v);
        if (at < cap) out_rows[at] = w * 64u + (uint32_t)b;   // (cap = the count the handle was created with: never exceeded)
        ++at;
        v &= v - 1ull;
    }
}

hipError_t launch_filter_row_list(const u64* words_dev, uint32_t nrows, uint32_t cap, uint32_t* scratch, uint32_t* out_rows,
                                  uint32_t* out_total, hipStream_t stream) {
    const uint32_t nwords = (nrows + 63u) / 64u;
    if (nwords == 0) return hipMemsetAsync(out_total, 0, 4, stream);
    const uint32_t nblocks = (nwords + kRowListWordsPerBlock - 1) / kRowListWordsPerBlock;
    uint32_t* word_off = scratch;             // [nwords]
    uint32_t* block_sum = scratch + nwords;   // [nblocks]
    hipLaunchKernelGGL(filter_row_list_count_kernel, dim3(nblocks), dim3(256), 0, stream, words_dev, nwords, nrows, word_off, block_sum);
    hipLaunchKernelGGL(filter_row_list_scan_kernel, dim3(1), dim3(256), 0, stream, block_sum, nblocks, out_total);
    hipLaunchKernelGGL(filter_row_list_expand_kernel, dim3((nwords + 255u) / 256u), dim3(256), 0, stream, words_dev, nwords, nrows,
                       (const uint32_t*)word_off, (const uint32_t*)block_sum, cap, out_rows);
    return hipGetLastError();
}

size_t filter_row_list_scratch_bytes(uint32_t nrows) {
    const size_t nwords = ((size_t)nrows + 63) / 64;
    return (nwords + (nwords + kRowListWordsPerBlock - 1) / kRowListWordsPerBlock + 1) * 4;
}

// ---- the segmented gather scan ------------------------------------------------------------------------------------------------------

// bytes between staged rows: row_bytes rounded so that pitch = 64 (mod 256)
__host__ __device__ inline uint32_t gather_row_pitch(uint32_t dim) {
    const uint32_t row_bytes = dim * 2u;
    return (row_bytes + 255u - 64u) / 256u * 256u + 64u;
}

size_t filter_gather_lds_bytes(uint32_t dim, int kcap) {
    return (size_t)kGatherTileRows * gather_row_pitch(dim)          // the tile
           + (size_t)kWavesPerBlock * dim * 4                       // a query per wave
           + (size_t)kWavesPerBlock * (2 * (size_t)kcap) * 8        // a candidate buffer per wave
           + (size_t)kGatherTileRows * 4;                           // the tile's row ids
}

template <int KCAP>
__global__ __launch_bounds__(256) void filter_gather_scan_kernel(FilterGatherArgs args) {
    constexpr int CAP = 2 * KCAP;
    constexpr int T = (int)kGatherTileRows;   // 64 rows: 16 quads x 4 rows per lane
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const FilterGatherGroup grp = args.groups[blockIdx.y];
    const uint32_t k = args.k;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, a = lane & 3, r = lane >> 2;
    const uint32_t ntiles = (grp.n + kGatherTileRows - 1) / kGatherTileRows;
    const uint32_t nblocks = grp.nblocks < ntiles ? grp.nblocks : ntiles;   // blocks of this group that own at least one tile
    // a block past its group's share still owns one list per query of the group: all empty (the merge reads gridDim.x lists per query)
    if (blockIdx.x >= nblocks) {
        for (uint32_t qi = 0; qi < grp.nq; ++qi) {
            u64* list = args.partial + ((size_t)(grp.q0 + qi) * gridDim.x + blockIdx.x) * args.list_stride;
            for (uint32_t i = tid; i < k; i += 256) list[i] = kEmpty;
        }
        return;
    }
    const uint32_t dim = args.dim;
    const uint32_t pitch = gather_row_pitch(dim);
    unsigned char* tile = smem;                                                         // [T][pitch]
    float* qs_all = reinterpret_cast<float*>(smem + (size_t)T * pitch);                 // [wave][dim]
    u64* bufs = reinterpret_cast<u64*>(qs_all + (size_t)kWavesPerBlock * dim);          // [wave][CAP]  (dim % 8 == 0: 16-byte aligned)
    uint32_t* s_row = reinterpret_cast<uint32_t*>(bufs + (size_t)kWavesPerBlock * CAP); // [T] local row, 0xffffffff = skip
    float* qs = qs_all + (size_t)wave * dim;
    u64* buf = bufs + (size_t)wave * CAP;

    const unsigned char* slab = reinterpret_cast<const unsigned char*>(args.slab);
    const uint32_t chunks = dim >> 3, groups = chunks >> 2, leftover = chunks & 3;
    bool first = true;
    for (uint32_t t = blockIdx.x; t < ntiles; t += nblocks) {
        __syncthreads();   // the previous tile has been read by every wave
        if (tid < T) {
            const uint32_t i = t * T + (uint32_t)tid;
            uint32_t row = 0xffffffffu;
            if (i < grp.n) {
                row = grp.rows[i];
                bool ok = row < args.nrows;
                if (ok && args.live) ok = (args.live[row >> 6] >> (row & 63u)) & 1ull;
                if (!ok) row = 0xffffffffu;
            }
            s_row[tid] = row;
        }
        __syncthreads();
        // stage the live rows: thread -> (row of the tile, 16-byte chunk), consecutive threads on consecutive chunks of a row
        for (uint32_t idx = tid; idx < (uint32_t)T * chunks; idx += 256) {
            const uint32_t i = idx / chunks, c = idx - i * chunks;
            const uint32_t row = s_row[i];
            if (row != 0xffffffffu) {
                const u32x4 w = *(reinterpret_cast<const u32x4*>(slab + (size_t)row * args.row_stride) + c);
                *reinterpret_cast<u32x4*>(tile + (size_t)i * pitch + (size_t)c * 16) = w;
            }
        }
        __syncthreads();
        const bool last = t + nblocks >= ntiles;   // the block's last tile: its lists go out best first
        for (uint32_t qi = wave; qi < grp.nq; qi += kWavesPerBlock) {
            const uint32_t slot = grp.q0 + qi;
            u64* list = args.partial + ((size_t)slot * gridDim.x + blockIdx.x) * args.list_stride;
            wave_lds_fence();   // the wave's previous query is done with qs and buf
            const float* qsrc = args.queries + (size_t)slot * dim;
            for (uint32_t i = lane; i < dim; i += 64) qs[i] = qsrc[i];
            // what the block holds for this query after its previous tiles — KCAP 64: one entry per lane (unordered, lanes below the
            // count), fetched now and needed only after the tile is scored
            u64 mine = kEmpty;
            if (KCAP == 64 && !first) mine = list[lane];
            WaveTopK<CAP> tk;
            tk.init(buf);
            u64 thr = 0;
            if (KCAP != 64 && !first) {   // KCAP 256: the best-first list this wave wrote after the previous tile, kEmpty behind the entries
                int have = 0;
                for (uint32_t i0 = 0; i0 < k; i0 += 64) {
                    const uint32_t i = i0 + lane;
                    const u64 e = i < k ? list[i] : kEmpty;
                    if (i < k) buf[i] = e;
                    have += (int)__popcll(__ballot(e != kEmpty));
                }
                tk.count = have;
                wave_lds_fence();
                if (have == (int)k) thr = sortkey(buf[k - 1]);
            }
            wave_lds_fence();
            float acc[4][8];
#pragma unroll
            for (int j = 0; j < 4; ++j)
#pragma unroll
                for (int x = 0; x < 8; ++x) acc[j][x] = 0.f;
            const unsigned char* trow = tile + (size_t)r * pitch;
            for (uint32_t g = 0; g < groups; ++g) {
                const float4* qp = reinterpret_cast<const float4*>(qs + 32 * g + 8 * a);
                const float4 q0 = qp[0], q1 = qp[1];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const u32x4 w = *(reinterpret_cast<const u32x4*>(trow + (size_t)(16 * j) * pitch) + 4 * g + a);
                    chunk_mac(acc[j], w, q0, q1);
                }
            }
            if (a == 0) {   // leftover chunks all accumulate into s0, in order
                for (uint32_t c = 4 * groups; c < 4 * groups + leftover; ++c) {
                    const float4* qp = reinterpret_cast<const float4*>(qs + 8 * c);
                    const float4 q0 = qp[0], q1 = qp[1];
#pragma unroll
                    for (int j = 0; j < 4; ++j) {
                        const u32x4 w = *(reinterpret_cast<const u32x4*>(trow + (size_t)(16 * j) * pitch) + c);
                        chunk_mac(acc[j], w, q0, q1);
                    }
                }
            }
            if constexpr (KCAP == 64) {
                // k <= 64: the k best so far sit one per lane; a row enters when it beats the worst of them (keys are unique, so
                // exactly one lane holds the worst).  No sort until the block's last tile.
                int count = (int)__popcll(__ballot(mine != kEmpty));
                auto worst = [&]() { return ~wave_max_key(lane < (int)k ? ~sortkey(mine) : 0ull); };
                if (count == (int)k) thr = worst();
                bool changed = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float score = quad_finish(acc[j], args.hreduce);
                    const uint32_t row = s_row[r + 16 * j];
                    const u64 packed = pack(score, args.row_base + row);
                    const bool cand = row != 0xffffffffu && a == 0 && sortkey(packed) > thr;
                    u64 m = __ballot(cand);
                    while (m) {   // wave-uniform: the candidates one after the other
                        const int src = __builtin_ctzll(m);
                        m &= m - 1ull;
                        const u64 c = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(packed >> 32), src) << 32) |
                                      (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)packed, src);
                        if (count < (int)k) {
                            if (lane == count) mine = c;
                            ++count;
                            changed = true;
                            if (count == (int)k) thr = worst();
                        } else if (sortkey(c) > thr) {
                            if (lane < (int)k && sortkey(mine) == thr) mine = c;
                            changed = true;
                            thr = worst();
                        }
                    }
                }
                if (last) {
                    buf[lane] = mine;
                    buf[64 + lane] = kEmpty;
                    wave_sort_desc<CAP>(buf, lane);
                    if (lane < (int)k) list[lane] = buf[lane];
                } else if (first || changed) {
                    list[lane] = mine;
                }
            } else {
                bool changed = false;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const float score = quad_finish(acc[j], args.hreduce);
                    const uint32_t row = s_row[r + 16 * j];
                    const u64 packed = pack(score, args.row_base + row);
                    bool cand = row != 0xffffffffu && a == 0 && sortkey(packed) > thr;
                    u64 m = __ballot(cand);
                    if (m == 0) continue;
                    changed = true;
                    if (tk.count + (int)__popcll(m) > CAP) {
                        thr = tk.compact((int)k, lane);
                        cand = cand && sortkey(packed) > thr;
                        m = __ballot(cand);
                    }
                    if (cand) buf[tk.count + (int)__popcll(m & ((1ull << lane) - 1ull))] = packed;
                    tk.count += (int)__popcll(m);
                }
                if (first || changed) {   // (nothing entered: the list in memory stands)
                    (void)tk.compact((int)k, lane);   // sorted, kEmpty behind the count
                    for (uint32_t i = lane; i < k; i += 64) list[i] = buf[i];
                }
            }
        }
        first = false;
        __threadfence_block();   // the lists are read back by the same wave, by other lanes
    }
}

template <int KCAP>
static hipError_t launch_filter_gather_t(const FilterGatherArgs& args, uint32_t ngroups, uint32_t grid_x, hipStream_t stream) {
    const size_t lds = filter_gather_lds_bytes(args.dim, KCAP);
    auto kern = filter_gather_scan_kernel<KCAP>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kern, dim3(grid_x, ngroups), dim3(256), lds, stream, args);
    return hipGetLastError();
}

bool filter_gather_supported(uint32_t dim, uint32_t k) {
    return dim >= 8 && dim % 8 == 0 && k >= 1 && k <= kGatherMaxK && filter_gather_lds_bytes(dim, k <= 64 ? 64 : 256) <= kGatherLdsBudget;
}

hipError_t launch_filter_gather_scan(const FilterGatherArgs& args, uint32_t ngroups, uint32_t grid_x, hipStream_t stream) {
    if (!filter_gather_supported(args.dim, args.k) || ngroups == 0 || ngroups > 65535 || grid_x == 0) return hipErrorInvalidValue;
    return args.k <= 64 ? launch_filter_gather_t<64>(args, ngroups, grid_x, stream) : launch_filter_gather_t<256>(args, ngroups, grid_x, stream);
}

}  // namespace fsgpu

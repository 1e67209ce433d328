// knn_optimize_kernels.hip — the k-NN graph optimisation (include/fsgpu.h, fsgpu_knn_graph_optimize): a table of
// neighbour ids in, a table of lower degree out; no vector is read and no distance computed, so every step is integer arithmetic
// and the result is a pure function of the table.
//   knn_opt_detour_kernel    one wave per source row x: the clean list C(x) into LDS with an id -> rank map, lane j walks the raw
//                            list of C(x)[j] and counts the detours x -> C(x)[j] -> C(x)[i] per rank i (LDS integer adds), the
//                            ranks are ordered by (count, rank) by counting and the first d written as F(x)
//   per rank r = 0 .. d - 1  knn_opt_keys_kernel (target << 32 | n - source; 0 for "no entry"), the library's radix sort
//                            (descending: targets descending, sources ASCENDING inside a target), knn_opt_place_kernel (a key's
//                            slot is fill[target] + its place in its run), knn_opt_advance_kernel (fill moves in a launch of its
//                            own: no key reads a count that a key of the same launch writes)
//   knn_opt_merge_kernel     one wave per row: F's first ceil(d / 2), the reverse candidates, the rest of F; first occurrences only
//   knn_opt_count_zero_kernel   the rows no edge points at (statistics only)
// The waves of a block work on separate rows and share nothing; they still meet at the block barriers, which order a wave's own
// LDS writes before its reads without leaning on the compiler.  The one-wave-per-row kernels run 2,048 blocks that stride over the
// rows, so that a block's statistics cost one atomic each (one per block of four rows was 30 ms of atomics at 10M rows).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef uint32_t ou32x4 __attribute__((ext_vector_type(4)));

constexpr uint32_t kMapSlots = 128;   // open addressing over at most 64 ids: half empty at worst
constexpr uint32_t kNoAdvance = 0xffffffffu;
constexpr uint64_t kOptMaxBlocks = 256 * 8;   // one-wave-per-row kernels: 8 blocks per CU stride over the rows

__device__ __forceinline__ uint32_t map_slot(uint32_t g) { return (g * 2654435761u) >> 25; }

template <bool VEC>
__global__ __launch_bounds__(256) void knn_opt_detour_kernel(KnnOptDetourArgs a) {
    __shared__ uint32_t s_raw[4][64], s_cid[4][64], s_cnt[4][64], s_key[4][kMapSlots], s_val[4][kMapSlots], s_max[4];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    uint32_t* raw = s_raw[wv];
    uint32_t* cid = s_cid[wv];
    uint32_t* cnt = s_cnt[wv];
    uint32_t* key = s_key[wv];
    uint32_t* val = s_val[wv];
    uint32_t block_max = 0;   // (thread 0's: one atomic per block, after its last row)

    // the blocks stride over the rows, four at a time; every wave of a block makes the same number of rounds (the barriers)
    for (uint64_t base = (uint64_t)blockIdx.x * 4u; base < a.n; base += (uint64_t)gridDim.x * 4u) {
        const uint64_t x64 = base + wv;
        const bool active = x64 < a.n;
        const uint32_t x = (uint32_t)x64;
        uint32_t g = kKnnPadRow;
        if (active && lane < a.width) g = a.table[x64 * a.width + lane];
        raw[lane] = g;
        cnt[lane] = 0;
        key[lane] = kKnnPadRow;
        key[lane + 64u] = kKnnPadRow;
        __syncthreads();

        // the clean list: up to the first pad, rows of the table only, not x, first occurrences only
        const unsigned long long pads = __ballot(g == kKnnPadRow);
        const uint32_t len = pads ? (uint32_t)(__ffsll(pads) - 1) : 64u;
        const uint32_t r = g - a.row_base;
        const bool valid = lane < len && g >= a.row_base && r < a.n && r != x;
        bool dup = false;
        for (uint32_t k = 0; k < len; ++k) dup |= k < lane && raw[k] == g;
        const bool keep = valid && !dup;
        const unsigned long long kept = __ballot(keep);
        const uint32_t nc = (uint32_t)__popcll(kept);
        const uint32_t rank = (uint32_t)__popcll(kept & ((1ull << lane) - 1ull));
        if (keep) {
            cid[rank] = g;
            uint32_t h = map_slot(g);
            while (atomicCAS(&key[h], kKnnPadRow, g) != kKnnPadRow) h = (h + 1u) & (kMapSlots - 1u);
            val[h] = rank;
        }
        // (every writer writes 1; a flag already seen set is not written again: the flags are read from cache, a store goes to memory)
        if (a.seen_before && valid && lane < a.degree && a.seen_before[r] == 0) a.seen_before[r] = 1;
        __syncthreads();

        // lane j walks the raw list of z = C(x)[j]: an id of C(x) met first at column p detours rank i when j < i and p < i.  i < nc,
        // so columns from nc - 1 on cannot count and are not read.
        if (lane + 1u < nc) {
            const uint32_t z = cid[lane] - a.row_base;
            const uint32_t* zr = a.table + (uint64_t)z * a.width;
            const uint32_t cols = a.width < nc - 1u ? a.width : nc - 1u;
            unsigned long long seen = 0;
            auto visit = [&](uint32_t gz, uint32_t p) {
                uint32_t h = map_slot(gz);
                for (uint32_t kk = key[h]; kk != kKnnPadRow; kk = key[h]) {
                    if (kk == gz) {
                        const uint32_t i = val[h];
                        if (!((seen >> i) & 1ull)) {
                            seen |= 1ull << i;
                            if (lane < i && p < i) atomicAdd(&cnt[i], 1u);
                        }
                        break;
                    }
                    h = (h + 1u) & (kMapSlots - 1u);
                }
            };
            if constexpr (VEC) {
                bool open = true;
                for (uint32_t p = 0; p < cols && open; p += 4u) {   // (width is a multiple of 4: the load stays inside the row)
                    const ou32x4 v = *reinterpret_cast<const ou32x4*>(zr + p);
#pragma unroll
                    for (uint32_t e = 0; e < 4u; ++e) {
                        if (open && v[e] == kKnnPadRow) open = false;
                        if (open && p + e < cols) visit(v[e], p + e);
                    }
                }
            } else {
                for (uint32_t p = 0; p < cols; ++p) {
                    const uint32_t gz = zr[p];
                    if (gz == kKnnPadRow) break;
                    visit(gz, p);
                }
            }
        }
        __syncthreads();

        // order the ranks by (count, rank): the place of rank i is the number of ranks whose pair is smaller
        uint32_t place = 64u, mine = 0;
        if (lane < nc) {
            mine = cnt[lane];
            const uint32_t me = (mine << 6) | lane;
            place = 0;
            for (uint32_t k = 0; k < nc; ++k) place += ((cnt[k] << 6) | k) < me ? 1u : 0u;
        }
        raw[lane] = kKnnPadRow;
        __syncthreads();
        if (lane < nc) raw[place] = cid[lane];
        if (a.max_detour) {
            for (int o = 32; o; o >>= 1) {
                const uint32_t other = (uint32_t)__shfl_xor((int)mine, o);
                mine = other > mine ? other : mine;
            }
            if (lane == 0) s_max[wv] = mine;
        }
        __syncthreads();
        if (active && lane < a.degree) a.fwd[x64 * a.degree + lane] = raw[lane];
        if (a.max_detour && threadIdx.x == 0)
            for (uint32_t k = 0; k < 4u; ++k) block_max = s_max[k] > block_max ? s_max[k] : block_max;
    }
    if (a.max_detour && threadIdx.x == 0 && block_max) atomicMax(a.max_detour, block_max);
}

__global__ __launch_bounds__(256) void knn_opt_keys_kernel(KnnOptRoundArgs a) {
    const uint64_t x = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (x >= a.n) return;
    const uint32_t g = a.fwd[x * a.degree + a.rank];
    a.keys[x] = g == kKnnPadRow ? 0ull : ((u64)(g - a.row_base) << 32) | (u64)(a.n - (uint32_t)x);
}

__global__ __launch_bounds__(256) void knn_opt_place_kernel(KnnOptRoundArgs a) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n) return;
    const u64 k = a.sorted[idx];
    uint32_t adv = kNoAdvance;
    if (k != 0ull) {
        const uint32_t y = (uint32_t)(k >> 32);
        const uint32_t f = a.fill[y];
        if (f < a.degree) {
            // the place in the run of y, as far as it matters: d - f predecessors of the same target put the key past the list
            uint32_t p = 0;
            while (p < a.degree - f && idx > p && (uint32_t)(a.sorted[idx - 1u - p] >> 32) == y) ++p;
            if (f + p < a.degree) {
                a.rev[(uint64_t)y * a.degree + f + p] = a.row_base + (a.n - (uint32_t)k);
                bool last = f + p + 1u == a.degree || idx + 1u == a.n;
                if (!last) {
                    const u64 nk = a.sorted[idx + 1u];
                    last = nk == 0ull || (uint32_t)(nk >> 32) != y;
                }
                if (last) adv = f + p + 1u;
            }
        }
    }
    a.advance[idx] = adv;
}

__global__ __launch_bounds__(256) void knn_opt_advance_kernel(KnnOptRoundArgs a) {
    const uint64_t idx = (uint64_t)blockIdx.x * 256u + threadIdx.x;
    if (idx >= a.n) return;
    const uint32_t adv = a.advance[idx];
    if (adv != kNoAdvance) a.fill[(uint32_t)(a.sorted[idx] >> 32)] = adv;   // one key per target and round
}

__global__ __launch_bounds__(256) void knn_opt_merge_kernel(KnnOptMergeArgs a) {
    __shared__ uint32_t s_seq[4][128], s_out[4][64], s_cnt[4][2];
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint32_t d = a.degree, h = (d + 1u) / 2u;
    uint32_t* seq = s_seq[wv];
    uint32_t* out = s_out[wv];
    u64 block_count = 0;   // (threads 0 and 1: entries from F, from the reverse candidates; one atomic each per block)

    for (uint64_t base = (uint64_t)blockIdx.x * 4u; base < a.n; base += (uint64_t)gridDim.x * 4u) {
        const uint64_t x64 = base + wv;
        const bool active = x64 < a.n;
        uint32_t f = kKnnPadRow, rv = kKnnPadRow, nr = 0;
        if (active && lane < d) f = a.fwd[x64 * d + lane];
        const uint32_t nf = (uint32_t)__popcll(__ballot(f != kKnnPadRow));   // F is dense: its entries are lanes 0 .. nf - 1
        if (active) {
            nr = a.fill[x64];
            nr = nr < d ? nr : d;
            if (lane < nr) rv = a.rev[x64 * d + lane];
        }
        // the sequence F[0, hf) | reverse candidates | F[hf, nf): at most 2 d <= 128 ids; the output is its first occurrences, cut at d
        const uint32_t hf = h < nf ? h : nf;
        if (lane < nf) seq[lane < hf ? lane : lane + nr] = f;
        if (lane < nr) seq[hf + lane] = rv;
        out[lane] = kKnnPadRow;
        __syncthreads();
        const uint32_t total = nf + nr;
        bool keep[2];
        uint32_t id[2];
#pragma unroll
        for (uint32_t half = 0; half < 2u; ++half) {
            const uint32_t q = lane + 64u * half;
            keep[half] = q < total;
            id[half] = keep[half] ? seq[q] : kKnnPadRow;
            if (keep[half] && q >= hf) {
                // a reverse candidate can repeat only one of the first hf, an entry of F's rest only a reverse candidate
                const uint32_t lo = q < hf + nr ? 0u : hf, hi = q < hf + nr ? hf : hf + nr;
                for (uint32_t k = lo; k < hi; ++k)
                    if (seq[k] == id[half]) keep[half] = false;
            }
        }
        const unsigned long long k0 = __ballot(keep[0]), k1 = __ballot(keep[1]);
        const unsigned long long below = (1ull << lane) - 1ull;
        const uint32_t at0 = (uint32_t)__popcll(k0 & below), at1 = (uint32_t)(__popcll(k0) + __popcll(k1 & below));
        bool rev_written[2];
#pragma unroll
        for (uint32_t half = 0; half < 2u; ++half) {
            const uint32_t q = lane + 64u * half, at = half ? at1 : at0;
            const bool w = keep[half] && at < d;
            if (w) out[at] = id[half];
            rev_written[half] = w && q >= hf && q < hf + nr;
            if (w && a.seen_after && a.seen_after[id[half] - a.row_base] == 0)   // (an entry of F or a source row: inside the table)
                a.seen_after[id[half] - a.row_base] = 1;
        }
        if (a.edge_counts) {
            uint32_t written = (uint32_t)(__popcll(k0) + __popcll(k1));
            written = written < d ? written : d;
            const uint32_t n_rev = (uint32_t)(__popcll(__ballot(rev_written[0])) + __popcll(__ballot(rev_written[1])));
            if (lane == 0) s_cnt[wv][0] = written - n_rev, s_cnt[wv][1] = n_rev;
        }
        __syncthreads();
        if (active && lane < d) a.out[x64 * d + lane] = out[lane];
        if (a.edge_counts && threadIdx.x < 2u)
            block_count += (u64)s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        __syncthreads();   // (the next round writes the lists and the counts again)
    }
    if (a.edge_counts && threadIdx.x < 2u && block_count)
        atomicAdd(reinterpret_cast<unsigned long long*>(a.edge_counts + threadIdx.x), (unsigned long long)block_count);
}

__global__ __launch_bounds__(256) void knn_opt_count_zero_kernel(const uint8_t* before, const uint8_t* after, uint64_t n, u64* out2) {
    __shared__ uint32_t s_part[4][2];
    uint32_t zb = 0, za = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256u) {
        zb += before[i] ? 0u : 1u;
        za += after[i] ? 0u : 1u;
    }
    for (int o = 32; o; o >>= 1) {
        zb += (uint32_t)__shfl_xor((int)zb, o);
        za += (uint32_t)__shfl_xor((int)za, o);
    }
    if ((threadIdx.x & 63u) == 0) s_part[threadIdx.x >> 6][0] = zb, s_part[threadIdx.x >> 6][1] = za;
    __syncthreads();
    if (threadIdx.x < 2u) {
        const u64 sum = (u64)s_part[0][threadIdx.x] + s_part[1][threadIdx.x] + s_part[2][threadIdx.x] + s_part[3][threadIdx.x];
        if (sum) atomicAdd(reinterpret_cast<unsigned long long*>(out2 + threadIdx.x), (unsigned long long)sum);
    }
}

bool shape_ok(uint64_t n, uint32_t width, uint32_t degree) {
    return n >= 1 && n <= 0xfffffffeull && degree >= 1 && degree <= width && width <= kKnnOptMaxWidth;
}

}  // namespace

hipError_t launch_knn_opt_detour(const KnnOptDetourArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (!shape_ok(a.n, a.width, a.degree)) return hipErrorInvalidValue;
    const uint64_t blocks = (a.n + 3u) / 4u;
    const dim3 grid((uint32_t)(blocks < kOptMaxBlocks ? blocks : kOptMaxBlocks)), block(256);
    const bool vec = a.width % 4u == 0 && (reinterpret_cast<uintptr_t>(a.table) & 15u) == 0;
    if (vec) hipLaunchKernelGGL(knn_opt_detour_kernel<true>, grid, block, 0, stream, a);
    else hipLaunchKernelGGL(knn_opt_detour_kernel<false>, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_knn_opt_round(const KnnOptRoundArgs& a, void* sort_temp, size_t sort_temp_bytes, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (!shape_ok(a.n, a.degree, a.degree) || a.rank >= a.degree) return hipErrorInvalidValue;
    const dim3 grid((uint32_t)((a.n + 255u) / 256u)), block(256);
    hipLaunchKernelGGL(knn_opt_keys_kernel, grid, block, 0, stream, a);
    // targets lie below n and n - source in 1 .. n: no bit above bit_width(n) of either half varies
    uint32_t bits = 0;
    while (bits < 32u && (a.n >> bits) != 0) ++bits;
    const u64 half = bits >= 32u ? 0xffffffffull : ((1ull << bits) - 1ull);
    hipError_t e = sort_keys_desc(sort_temp, sort_temp_bytes, a.keys, a.sorted, (size_t)a.n, stream, (half << 32) | half);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(knn_opt_place_kernel, grid, block, 0, stream, a);
    hipLaunchKernelGGL(knn_opt_advance_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_knn_opt_merge(const KnnOptMergeArgs& a, hipStream_t stream) {
    if (a.n == 0) return hipSuccess;
    if (!shape_ok(a.n, a.degree, a.degree)) return hipErrorInvalidValue;
    const uint64_t blocks = (a.n + 3u) / 4u;
    hipLaunchKernelGGL(knn_opt_merge_kernel, dim3((uint32_t)(blocks < kOptMaxBlocks ? blocks : kOptMaxBlocks)), dim3(256), 0, stream, a);
    return hipGetLastError();
}

hipError_t launch_knn_opt_count_zero(const uint8_t* before, const uint8_t* after, uint64_t n, u64* out2, hipStream_t stream) {
    if (n == 0) return hipSuccess;
    const uint64_t blocks = (n + 255u) / 256u;
    hipLaunchKernelGGL(knn_opt_count_zero_kernel, dim3((uint32_t)(blocks < 2048u ? blocks : 2048u)), dim3(256), 0, stream, before, after, n, out2);
    return hipGetLastError();
}

}  // namespace fsgpu

// ivf_filter_kernels.hip — the int8 matrix-core list filter of the inverted-file index (kernels.hpp; ivf_index.cpp).
//
//   ivf_filter_gather_kernel   the cluster-ordered copy of the index's int8 filter rows: once per handle, HBM-bound
//   ivf_filter_score_kernel    v_mfma_i32_16x16x64_i8 over (list, tile of <= 16 member queries, 512 rows): every probed list is scored
//                              once for all the queries that probe it, EXACT integer dots into a per-slot scratch
//   ivf_filter_select_kernel   per slot: the k-th largest score (a radix select, four 8-bit digits), the margin, the ordered compaction
//
// Nothing here depends on the order in which waves or workgroups run: the scratch entry of a (slot, row) has one writer, the
// selection's histograms are integer counts, and the compaction places a candidate by a prefix sum over its position in the list.
#include "device_util.hpp"
#include "kernels.hpp"

namespace fsgpu {

namespace {

typedef int i32x4 __attribute__((ext_vector_type(4)));

// One thread per 8 bytes of a logical row (dim % 8 == 0): the list by a binary search of the offsets.
__global__ __launch_bounds__(256) void ivf_filter_gather_kernel(const signed char* __restrict__ src, uint32_t dim, const uint32_t* __restrict__ list_rows,
                                                                const u64* __restrict__ offsets, const u64* __restrict__ pad_row0, uint32_t nlist,
                                                                u64 total, uint32_t pitch, signed char* __restrict__ dst) {
    const uint32_t chunks = dim >> 3;
    const u64 gid = (u64)blockIdx.x * 256u + threadIdx.x;
    const u64 p = gid / chunks;
    if (p >= total) return;
    const uint32_t c = (uint32_t)(gid - p * chunks);
    uint32_t lo = 0, hi = nlist;   // the list l with offsets[l] <= p < offsets[l + 1]: the last l with offsets[l] <= p
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (offsets[mid] <= p) lo = mid;
        else hi = mid;
    }
    const u64 row = list_rows[p];
    const uint2 v = *reinterpret_cast<const uint2*>(src + row * dim + (size_t)c * 8);
    *reinterpret_cast<uint2*>(dst + (pad_row0[lo] + (p - offsets[lo])) * pitch + (size_t)c * 8) = v;
}

// 256 threads, four waves.  The tile's codes sit in LDS, pitch + 32 bytes apart (mfma_scan.hip: a 32-byte pad keeps ds_read_b128
// conflict-free); rows of queries past the tile's members are zero.  A wave takes the 16-row tiles w, w + 4, ... of the item's 512 rows:
// A = 16 rows x 64 codes (lane: row lane & 15, bytes 16 (lane >> 4) .. of the k-step), B = the 16 queries alike, C: column (query)
// lane & 15, rows 4 (lane >> 4) + r.
__global__ __launch_bounds__(256) void ivf_filter_score_kernel(IvfFilterScoreArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t item = a.item_first + blockIdx.x;
    // the tile: the last t of the launch's tiles with item0 <= item (every tile of a range owns at least one item)
    uint32_t lo = a.tile_first, hi = a.tile_first + a.ntiles;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (a.tiles[mid].item0 <= item) lo = mid;
        else hi = mid;
    }
    const IvfFilterTile t = a.tiles[lo];
    const uint32_t pitch = a.pitch, qpitch = pitch + 32;
    {   // stage the member queries' codes: 8-byte pieces; zero behind dim and for the rows past the members
        const uint32_t pieces = pitch >> 3, dpieces = a.dim >> 3;
        for (uint32_t i = tid; i < kIvfFilterTileQueries * pieces; i += 256) {
            const uint32_t q = i / pieces, p = i - q * pieces;
            uint2 v = make_uint2(0u, 0u);
            if (q < t.nmem && p < dpieces) v = *reinterpret_cast<const uint2*>(a.codes + (size_t)a.slot_query[t.slot0 + q] * a.dim + (size_t)p * 8);
            *reinterpret_cast<uint2*>(smem + (size_t)q * qpitch + (size_t)p * 8) = v;
        }
    }
    __syncthreads();
    const uint32_t len_pad = (t.len + kIvfFilterRowTile - 1) / kIvfFilterRowTile * kIvfFilterRowTile;
    const uint32_t row_begin = (item - t.item0) * kIvfFilterItemRows;
    const uint32_t row_end = row_begin + kIvfFilterItemRows < len_pad ? row_begin + kIvfFilterItemRows : len_pad;
    const int frow = lane & 15, fk = lane >> 4;
    const uint32_t ksteps = pitch >> 6;
    const unsigned char* bq = smem + (size_t)frow * qpitch + (size_t)fk * 16;
    for (uint32_t r0 = row_begin + (uint32_t)wave * 16u; r0 < row_end; r0 += 64u) {
        // (the ordered copy holds len_pad rows of this list: every row read here exists)
        const signed char* ar = a.ordered + (t.ordered_row0 + r0 + (uint32_t)frow) * pitch + (size_t)fk * 16;
        i32x4 acc = {0, 0, 0, 0};
        for (uint32_t ks = 0; ks < ksteps; ++ks) {
            const i32x4 av = *reinterpret_cast<const i32x4*>(ar + (size_t)ks * 64);
            const i32x4 bv = *reinterpret_cast<const i32x4*>(bq + (size_t)ks * 64);
            acc = __builtin_amdgcn_mfma_i32_16x16x64_i8(av, bv, acc, 0, 0, 0);
        }
        // the lane's four rows of its query: dead rows and the padding take the sentinel
        const uint32_t i0 = r0 + (uint32_t)fk * 4u;
        i32x4 out;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const uint32_t i = i0 + (uint32_t)r;
            bool live = false;
            if (i < t.len) live = row_live(a.live, a.list_rows[t.list_pos0 + i]);
            out[r] = live ? acc[r] : kIvfFilterDead;
        }
        if ((uint32_t)frow < t.nmem)   // scratch0 and len_pad are multiples of 4 entries: one 16-byte store
            *reinterpret_cast<i32x4*>(a.scores + t.scratch0 + (size_t)frow * len_pad + i0) = out;
    }
}

// One workgroup per slot.  The keys are the scores with the sign bit flipped (unsigned order = signed order); the dead rows' key is 0.
__global__ __launch_bounds__(256) void ivf_filter_select_kernel(IvfFilterSelectArgs a) {
    __shared__ uint32_t hist[256];
    __shared__ uint32_t s_pick[2];   // the digit chosen and what remains of k below the digits above it
    __shared__ uint32_t wsum[4];
    const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint32_t slot = a.slot_first + blockIdx.x;
    const float delta = a.delta[a.slot_query[slot]];
    if (!(delta >= 0.0f)) {   // (block-uniform) not certified: the whole list is scanned
        if (tid == 0) {
            a.out_t[slot] = kIvfFilterDead;
            a.out_m[slot] = 0;
            a.out_count[slot] = 0;
            a.out_flag[slot] = kIvfFilterFlagUncertified;
        }
        return;
    }
    const uint32_t tile = a.slot_tile[slot];
    const IvfFilterTile t = a.tiles[tile];
    const uint32_t len_pad = (t.len + kIvfFilterRowTile - 1) / kIvfFilterRowTile * kIvfFilterRowTile;
    const int32_t* s = a.scores + t.scratch0 + (size_t)(slot - t.slot0) * len_pad;
    const uint32_t k = a.k;
    // the live rows
    int mine = 0;
    for (uint32_t i = tid; i < t.len; i += 256) mine += s[i] != kIvfFilterDead;
    uint32_t nlive = 0;
    {
        for (int off = 32; off > 0; off >>= 1) mine += __shfl_xor(mine, off);
        if (lane == 0) wsum[wave] = (uint32_t)mine;
        __syncthreads();
        nlive = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        __syncthreads();
    }
    const long long m = (long long)ceil(2.0 * (double)delta);
    int32_t tk = kIvfFilterDead;
    if (nlive > k) {
        // the k-th largest key, a digit at a time from the top: the histogram of the digit among the keys that share the prefix
        uint32_t prefix = 0, remaining = k;
        for (int shift = 24; shift >= 0; shift -= 8) {
            hist[tid] = 0;
            __syncthreads();
            const uint32_t mask = shift == 24 ? 0u : ~0u << (shift + 8);
            for (uint32_t i = tid; i < t.len; i += 256) {
                const uint32_t key = (uint32_t)s[i] ^ 0x80000000u;
                if ((key & mask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
            }
            __syncthreads();
            if (wave == 0) {
                // the bin that holds the remaining-th largest key: a lane owns four bins, a suffix sum over the lanes finds the one
                // lane whose bins straddle it (the keys under the prefix number at least `remaining`: exactly one lane qualifies)
                uint32_t h[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) h[j] = hist[4 * lane + j];
                const uint32_t c = h[0] + h[1] + h[2] + h[3];
                uint32_t incl = c;   // keys in this lane's bins and in every higher lane's
                for (int off = 1; off < 64; off <<= 1) {
                    const uint32_t v = __shfl_down(incl, off);
                    if (lane + off < 64) incl += v;
                }
                const uint32_t above = incl - c;
                if (above < remaining && remaining <= incl) {
                    uint32_t rem = remaining - above, d = 3;   // (constant indexes: h stays in registers)
                    if (h[3] < rem) {
                        rem -= h[3], d = 2;
                        if (h[2] < rem) {
                            rem -= h[2], d = 1;
                            if (h[1] < rem) rem -= h[1], d = 0;
                        }
                    }
                    s_pick[0] = 4u * (uint32_t)lane + d;
                    s_pick[1] = rem;
                }
            }
            __syncthreads();
            prefix |= s_pick[0] << shift;
            remaining = s_pick[1];
            __syncthreads();
        }
        tk = (int32_t)(prefix ^ 0x80000000u);
    }
    // the candidates, ascending: a live row when no more than k are live, else s >= t - m
    const long long thr = nlive > k ? (long long)tk - m : (long long)kIvfFilterDead + 1;
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < t.len; i0 += 256) {
        const uint32_t i = i0 + (uint32_t)tid;
        bool take = false;
        if (i < t.len) {
            const int32_t v = s[i];
            take = v != kIvfFilterDead && (long long)v >= thr;
        }
        const u64 ballot = __ballot(take);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t before = 0;
        for (int w = 0; w < wave; ++w) before += wsum[w];
        const uint32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        const uint32_t pos = base + before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (take && pos < kIvfFilterSlotCap) a.cand[(size_t)slot * kIvfFilterSlotCap + pos] = a.list_rows[t.list_pos0 + i];
        base += total;
        __syncthreads();
    }
    if (tid == 0) {
        a.out_t[slot] = tk;
        a.out_m[slot] = m;
        a.out_count[slot] = base;
        a.out_flag[slot] = base > kIvfFilterSlotCap ? kIvfFilterFlagOverflow : 0u;
    }
}

}  // namespace

hipError_t launch_ivf_filter_gather(const signed char* filter_i8, uint32_t dim, const uint32_t* list_rows, const u64* offsets, const u64* pad_row0,
                                    uint32_t nlist, uint64_t total, uint32_t pitch, signed char* ordered, hipStream_t stream) {
    if (total == 0) return hipSuccess;
    if (dim < 8 || dim % 8 != 0 || pitch < dim || pitch % kIvfFilterPitchAlign != 0 || nlist < 1) return hipErrorInvalidValue;
    const uint64_t threads = total * (dim >> 3), blocks = (threads + 255) / 256;
    if (blocks > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_filter_gather_kernel, dim3((uint32_t)blocks), dim3(256), 0, stream, filter_i8, dim, list_rows, offsets, pad_row0, nlist,
                       (u64)total, pitch, ordered);
    return hipGetLastError();
}

hipError_t launch_ivf_filter_score(const IvfFilterScoreArgs& a, uint32_t nitems, hipStream_t stream) {
    if (nitems == 0 || a.ntiles == 0) return hipSuccess;
    if (a.dim < 8 || a.dim % 8 != 0 || a.pitch < a.dim || a.pitch % kIvfFilterPitchAlign != 0 || nitems > 0x7fffffffu) return hipErrorInvalidValue;
    const size_t lds = (size_t)kIvfFilterTileQueries * (a.pitch + 32);
    if (lds > 64 * 1024) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_filter_score_kernel, dim3(nitems), dim3(256), lds, stream, a);
    return hipGetLastError();
}

hipError_t launch_ivf_filter_select(const IvfFilterSelectArgs& a, uint32_t nslots, hipStream_t stream) {
    if (nslots == 0) return hipSuccess;
    if (a.k < 1 || a.k > kIvfFilterKCap || nslots > 0x7fffffffu) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ivf_filter_select_kernel, dim3(nslots), dim3(256), 0, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu

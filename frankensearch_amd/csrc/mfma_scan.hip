// mfma_scan.hip — batched f16 cosine scan on the matrix cores: 64 or 128 queries per pass over the slab, with
// results that are still BIT-IDENTICAL to the reference CPU path.
//
// The exact VALU kernels (scan_kernels.hip, scan_mq_kernel.hip) reproduce the reference's f32 operation order and
// top out at 4-8 queries per HBM pass.  Here the contraction slab[rows,dim] x queries[dim,NQ] runs on
// v_mfma_f32_16x16x32_f16 with the queries rounded to f16, which gives only APPROXIMATE scores a(r,q).  Exactness
// is recovered by a provable filter + exact re-score (the same pass-1 / pass-2 shape the reference ships for int8,
// crates/frankensearch-index/src/search.rs:589-661):
//
//   |a(r,q) - s(r,q)| <= delta_q = (2^-11 (1+2^-11) + dim 2^-23) * max_row_norm * |q| + sqrt(dim) 2^-25 * max_row_norm
//       (f16 rounding of the query: relative 2^-11 per element, Cauchy-Schwarz over the row; f32 accumulation of
//        exact f16 x f16 products inside the MFMA; f16-subnormal query elements)
//   so every true top-k row has a >= a_k - 2 delta_q, where a_k is the k-th largest approximate score of ANY
//   subset of rows (a subset's k-th best is a lower bound of the corpus' k-th best).
//
// Pipeline per group of 64 / 128 queries (host side: VectorIndex::search_top_k_batched_device):
//   stage A  dense approximate scores of a 4096-row sample        -> select: tau_q = a_k - 2 delta_q
//   stage B  a ~N/64-row sample (superset of A), rows with a >= tau_q kept -> select: tighter tau_q + candidate pool
//   stage C  every row B did not visit, with the final tau_q (a few hundred survivors per query out of 10M rows)
//   finish   a_k over pool + survivors; the rows with a >= a_k - 2 delta_q (at most kSelectPool, else the query is
//            handed to the exact kernels) are re-scored with the exact-order dot inside the block and the best k
//            exact entries are emitted: rows AND score bits equal the exact path's.
//   The samples are 64-row groups spread evenly over the slab, so tau is representative even when neighbouring
//   rows are correlated.  Candidates are staged in LDS and written as one short list per (query, block): appending
//   through global atomics serialises on the counter's cache line (~0.18 us per append, measured).
//
// Kernel mapping: a wave owns 16- or 32-row tiles (12/24 KB at dim 384); loads use the coalesced quad layout of the
// exact kernels and are transposed into the MFMA's A-fragment layout with ds_bpermute; the f16 queries sit in LDS
// ([NQ][dim+8] halves: the 16-byte pad staggers rows across banks) and are read as B fragments with one
// ds_read_b128 per (k-step, query tile), each feeding one MFMA per 16-row sub-tile.  Algorithmic bytes per pass are
// still N*dim*2.  At 64 queries the kernel is HBM-bound; at 128 queries the B-fragment reads (96 KB of LDS traffic
// per 16 rows) bound the 16-row tiling, the 32-row tiling halves them and is HBM-bound again.
#include <atomic>
#include <cstdlib>
#include <string>
#include <type_traits>

#include "scan_common.hpp"

namespace fsgpu {

using namespace scan_detail;

typedef float f32x4 __attribute__((ext_vector_type(4)));

// STAGE only separates the kernel symbols (0 = dense sample, 1 = bounded range, 2 = main pass) so profiles report the
// dominant main-pass launches on their own; 0 also makes the dense branch compile-time.
// EB = bytes per slab element: 2 = f16 rows against f16-rounded queries (v_mfma_f32_16x16x32_f16, approximate scores),
// 1 = the int8 slab against int8 queries (v_mfma_i32_16x16x64_i8, EXACT integer scores: the reference's int8 pass 1,
// search.rs:589-661).  Everything else is byte-level and shared: a lane's 16-byte fragment is 8 halves or 16 int8.
template <int DIM_E, int NQT, int WPB, int STAGE, int RT, bool PF, int EB = 2>
__global__ __launch_bounds__(WPB * 64) void scan_mfma_kernel(MfmaScanArgs args) {
    constexpr int DIM = DIM_E * EB / 2;  // row length in 2-byte units
    typedef int i32x4 __attribute__((ext_vector_type(4)));
    using acc_t = std::conditional_t<EB == 2, f32x4, i32x4>;
    constexpr int NT = WPB * 64;
    constexpr int KS = DIM / 32;        // MFMA k-steps
    // halves per query row in LDS: a 32-byte pad.  ds_read_b128 is served in four 16-lane groups that are NOT contiguous
    // ({0-3,12-15,20-27}, ...; MI355X_MICROARCH.md, LDS): with fragment addresses row * pitch + kgroup * 16 a group is
    // conflict-free iff (pitch / 16) mod 16 is 2, 6, 10 or 14.  A 16-byte pad (pitch/16 = 1 mod 16) is 2-way conflicted in
    // every group: SQ_LDS_BANK_CONFLICT was 43 % of SQ_LDS_IDX_ACTIVE on the main pass.
    constexpr int QSTRIDE = DIM + 16;
    constexpr int NQ = NQT * 16;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    _Float16* qs = reinterpret_cast<_Float16*>(smem);
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);  // scalar: the tile index arithmetic stays on the SALU
    const int frow = lane & 15;  // A: row inside the tile / B: query inside the query tile / C: column (query)
    const int fk = lane >> 4;    // k-group (8 halves each) / C: row group (4 rows each)
    if (gridDim.y > 1) {
        // several query groups in one launch (the sample stages of a large batch): blockIdx.y picks the group, whose
        // per-query arrays follow the previous group's
        const size_t grp = blockIdx.y;
        args.queries = static_cast<const unsigned char*>(args.queries) + grp * NQ * (size_t)DIM * 2;
        args.tau += grp * NQ;
        if (STAGE == 0) {
            args.dense += grp * NQ * (size_t)args.group_count * 64;
        } else {
            args.cand += grp * NQ * (size_t)gridDim.x * args.slots;
            args.spill += grp * NQ * (size_t)args.spill_cap;
            args.spill_count += grp * NQ * kMfmaSpillCountStride;
            args.overflow += grp * NQ;
        }
    }
    {   // stage the queries: 16-byte pieces, coalesced
        const u32x4* src = static_cast<const u32x4*>(args.queries);
        constexpr int PIECES = DIM / 8;
        for (int i = tid; i < NQ * PIECES; i += NT) {
            const int q = i / PIECES, p = i - q * PIECES;
            *reinterpret_cast<u32x4*>(qs + (size_t)q * QSTRIDE + p * 8) = src[(size_t)q * PIECES + p];
        }
    }
    // per-block candidate staging (stages 1/2): LDS atomics only; one global list per (query, block) is written at
    // the end.  (Appending through global atomics serialises on the per-query counter: ~0.18 us per append.)
    int* lcnt = reinterpret_cast<int*>(smem + (size_t)NQ * QSTRIDE * 2);
    u64* lbuf = reinterpret_cast<u64*>(smem + (size_t)NQ * QSTRIDE * 2 + (size_t)NQ * 4);
    const int slots = (int)args.slots;
    if (STAGE != 0) {
        for (int i = tid; i < NQ; i += NT) lcnt[i] = 0;
        for (int i = tid; i < NQ * slots; i += NT) lbuf[i] = kEmpty;
    }
    __syncthreads();
    float tau[NQT];
#pragma unroll
    for (int nt = 0; nt < NQT; ++nt) tau[nt] = STAGE == 0 ? -INFINITY : args.tau[nt * 16 + frow];

    // A wave iteration covers RT consecutive 16-row sub-tiles: every B fragment read from LDS feeds RT MFMAs, so
    // the LDS traffic per row falls by RT (at 128 queries the B reads, 96 KB per 16 rows, are what bounds RT = 1).
    constexpr uint32_t TROWS = 16 * RT;
    constexpr uint32_t TPG = 64 / TROWS;  // tiles per 64-row group (one live/allow bitmap word)
    // Row coverage, in 64-row groups.  Sample launches (stages 0/1) visit groups {j * group_stride : j < group_count},
    // spread over the whole slab so that the threshold they produce is representative even when neighbouring rows are
    // correlated (documents arrive in topical runs); the main pass (stage 2) visits every group that stage 1 did not.
    const uint32_t ntiles = STAGE == 2 ? (args.nrows + TROWS - 1) / TROWS : args.group_count * TPG;
    const uint32_t nwaves = gridDim.x * WPB;
    const unsigned char* slab = reinterpret_cast<const unsigned char*>(args.slab);
    const size_t row_bytes = args.row_stride ? (size_t)args.row_stride : (size_t)DIM * 2;
    const uint32_t last_row = args.nrows - 1;
    auto tile_row0 = [&](uint32_t t) -> uint32_t {
        if (STAGE == 2) return t * TROWS;
        return (t / TPG) * args.group_stride * 64 + (t % TPG) * TROWS;
    };
    auto tile_skipped = [&](uint32_t t) -> bool {  // main pass: the group was covered by the stage-1 sample
        if (STAGE != 2) return false;
        const uint32_t g = (t * TROWS) >> 6;
        const uint32_t j = g / args.group_stride;
        return j * args.group_stride == g && j < args.group_count;
    };

    // HBM side: the coalesced quad layout of the exact kernels — lane (r = lane>>2, a = lane&3) fetches chunk 4ks+a
    // of row r, so four consecutive lanes read 64 contiguous bytes.  The MFMA wants lane (row = lane&15,
    // k-group = lane>>4) instead; loading in that shape directly costs 4x the address-coalescer work (every group of
    // 16 lanes would touch 16 rows) and was measured at 0.46 of HBM peak.  The fragments are therefore transposed
    // across lanes with ds_bpermute right before use: destination lane d reads source lane ((d&15)<<2)|(d>>4).
    const int lrow = lane >> 2, lchunk = lane & 3;
    const int perm_addr = ((((lane & 15) << 2) | (lane >> 4)) << 2);  // byte address for ds_bpermute
    auto load_tile = [&](uint32_t t, half8 (&w)[RT][KS]) {
#pragma unroll
        for (int s = 0; s < RT; ++s) {
            uint32_t row = tile_row0(t) + s * 16 + lrow;
            row = row < args.nrows ? row : last_row;
            const half8* p = reinterpret_cast<const half8*>(slab + (size_t)row * row_bytes) + lchunk;
#pragma unroll
            for (int ks = 0; ks < KS; ++ks) w[s][ks] = p[ks * 4];
        }
    };
    auto to_fragment = [&](const half8& v) {
        typedef int i32x4 __attribute__((ext_vector_type(4)));
        const i32x4 x = __builtin_bit_cast(i32x4, v);
        i32x4 y;
        y[0] = __builtin_amdgcn_ds_bpermute(perm_addr, x[0]);
        y[1] = __builtin_amdgcn_ds_bpermute(perm_addr, x[1]);
        y[2] = __builtin_amdgcn_ds_bpermute(perm_addr, x[2]);
        y[3] = __builtin_amdgcn_ds_bpermute(perm_addr, x[3]);
        return __builtin_bit_cast(half8, y);
    };
    auto tile_words = [&](uint32_t t, u64& live_word, u64& allow_word) {
        const uint32_t w64 = tile_row0(t) >> 6;
        live_word = args.live ? args.live[w64] : ~0ull;
        allow_word = args.allow ? args.allow[w64] : ~0ull;
    };
    auto compute_tile = [&](uint32_t t, const half8 (&w)[RT][KS], u64 live_word, u64 allow_word) {
        acc_t acc[RT][NQT];
#pragma unroll
        for (int s = 0; s < RT; ++s)
#pragma unroll
            for (int nt = 0; nt < NQT; ++nt) acc[s][nt] = acc_t{0, 0, 0, 0};
#pragma unroll
        for (int ks = 0; ks < KS; ++ks) {
            half8 afrag[RT];
#pragma unroll
            for (int s = 0; s < RT; ++s) afrag[s] = to_fragment(w[s][ks]);
#pragma unroll
            for (int nt = 0; nt < NQT; ++nt) {
                const half8 b = *reinterpret_cast<const half8*>(qs + (size_t)(nt * 16 + frow) * QSTRIDE + ks * 32 + fk * 8);
#pragma unroll
                for (int s = 0; s < RT; ++s)
                    if constexpr (EB == 2)
                        acc[s][nt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(afrag[s], b, acc[s][nt], 0, 0, 0);
                    else
                        acc[s][nt] = __builtin_amdgcn_mfma_i32_16x16x64_i8(__builtin_bit_cast(i32x4, afrag[s]),
                                                                           __builtin_bit_cast(i32x4, b), acc[s][nt], 0, 0, 0);
            }
            // keep the B-fragment reads of later k-steps below this point: unconstrained, hipcc hoists all KS*NQT
            // ds_read_b128 to the top of the tile (192 extra registers at dim 384 -> one wave per SIMD)
#pragma unroll
            for (int s = 0; s < RT; ++s)
#pragma unroll
                for (int nt = 0; nt < NQT; ++nt) asm volatile("" : "+v"(acc[s][nt])::"memory");
        }
#pragma unroll
        for (int s = 0; s < RT; ++s) {
            // C layout: column (query) = lane & 15, row = (lane >> 4) * 4 + reg
            const uint32_t row0 = tile_row0(t) + s * 16 + fk * 4;
            bool valid[4];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const uint32_t row = row0 + r;
                valid[r] = row < args.nrows && ((live_word >> (row & 63)) & 1ull) && ((allow_word >> (row & 63)) & 1ull);
            }
            if constexpr (STAGE == 0) {
                const size_t span = (size_t)args.group_count * 64;  // dense slot = position inside the sample
                const uint32_t pos0 = t * TROWS + s * 16 + fk * 4;
#pragma unroll
                for (int nt = 0; nt < NQT; ++nt)
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        args.dense[(size_t)(nt * 16 + frow) * span + pos0 + r] =
                            valid[r] ? pack((float)acc[s][nt][r], args.row_base + row0 + r) : kEmpty;
            } else {
#pragma unroll
                for (int nt = 0; nt < NQT; ++nt) {
                    const float th = tau[nt];
                    // cheap reject first: the best of the lane's four rows against the threshold (max ignores NaN);
                    // survivors are a few hundred rows out of the whole slab
                    // (fmaxf, not a comparison chain: `a > NaN ? a : NaN` keeps the NaN, and a row with a NaN element — its score is
                    // NaN, it ranks last — would take the three rows that share its lane down with it)
                    auto m = acc[s][nt][0];
#pragma unroll
                    for (int r = 1; r < 4; ++r) {
                        if constexpr (EB == 2) m = __builtin_fmaxf(m, acc[s][nt][r]);
                        else m = acc[s][nt][r] > m ? acc[s][nt][r] : m;
                    }
                    if (__builtin_expect(!((float)m >= th), 1)) continue;   // (expected: the append code goes out of line, the tile loop falls through)
                    const int q = nt * 16 + frow;
#pragma unroll
                    for (int r = 0; r < 4; ++r)
                        if (valid[r] && (float)acc[s][nt][r] >= th) {
                            const int pos = atomicAdd(&lcnt[q], 1);
                            const u64 entry = pack((float)acc[s][nt][r], args.row_base + row0 + r);
                            if (pos < slots) {
                                lbuf[q * slots + pos] = entry;
                            } else {
                                // the block's list is full: spill to the query's global overflow area (rare, so the
                                // serialised global atomic does not matter); beyond that the exact path answers
                                const uint32_t g = atomicAdd(&args.spill_count[q * kMfmaSpillCountStride], 1u);
                                if (g < args.spill_cap) args.spill[(size_t)q * args.spill_cap + g] = entry;
                                else args.overflow[q] = 1;
                            }
                        }
                }
            }
        }
    };

    // Work item u = round * gridDim.x + block; the tile it names is rotated by the round number inside its round:
    // tile = round * grid + (block - round) mod grid.  Neighbouring tiles go to different blocks (a run of
    // neighbouring rows — one topic's documents, typically where a query's candidates cluster — is spread over many
    // blocks' candidate lists), and rows that recur with a power-of-two period do not keep landing in the same blocks.
    const uint32_t grid = gridDim.x;
    const uint32_t nitems = (ntiles + grid - 1) / grid * grid;
    auto tile_of = [&](uint32_t u) -> uint32_t {
        const uint32_t round = u / grid, blk = u - round * grid;
        const uint32_t rot = round % grid;
        const uint32_t t = round * grid + (blk >= rot ? blk - rot : blk + grid - rot);
        return args.reverse ? nitems - 1 - t : t;  // items past the last tile are skipped either way
    };
    auto next_item = [&](uint32_t u) -> uint32_t {  // the wave's next work item at or after u that names a tile to scan
        while (u < nitems) {
            const uint32_t t = tile_of(u);
            if (t < ntiles && !tile_skipped(t)) break;
            u += nwaves;
        }
        return u;
    };
    const uint32_t u0 = wave * grid + blockIdx.x;
    if constexpr (PF) {
        // register double buffer: the next tile's loads are in flight while this one is on the matrix cores
        half8 wa[RT][KS], wb[RT][KS];
        u64 la = ~0ull, aa = ~0ull, lb = ~0ull, ab = ~0ull;
        uint32_t u = next_item(u0);
        if (u < nitems) {
            load_tile(tile_of(u), wa);
            tile_words(tile_of(u), la, aa);
        }
        while (u < nitems) {
            uint32_t next = next_item(u + nwaves);
            if (next < nitems) {
                load_tile(tile_of(next), wb);
                tile_words(tile_of(next), lb, ab);
            }
            compute_tile(tile_of(u), wa, la, aa);
            u = next;
            if (u >= nitems) break;
            next = next_item(u + nwaves);
            if (next < nitems) {
                load_tile(tile_of(next), wa);
                tile_words(tile_of(next), la, aa);
            }
            compute_tile(tile_of(u), wb, lb, ab);
            u = next;
        }
    } else {
        // single buffer: the other resident waves of the SIMD cover the load latency
        half8 wa[RT][KS];
        u64 la = ~0ull, aa = ~0ull;
        for (uint32_t u = next_item(u0); u < nitems; u = next_item(u + nwaves)) {
            const uint32_t t = tile_of(u);
            load_tile(t, wa);
            tile_words(t, la, aa);
            compute_tile(t, wa, la, aa);
        }
    }
    if (STAGE != 0) {
        __syncthreads();
        // one list of `slots` entries per (query, block), kEmpty padded: [q][block][slots]
        for (int i = tid; i < NQ * slots; i += NT) {
            const int q = i / slots, j = i - q * slots;
            args.cand[((size_t)q * gridDim.x + blockIdx.x) * slots + j] = lbuf[i];
        }
    }
}

// Selection without a full sort (see SelectArgs).  1024 threads hold 8 entries each in registers (8,192 per pass;
// longer inputs take more passes); every wave keeps its k largest sortkeys so far (wave_extract_topk over its new
// entries plus its previous winners), wave 0 repeats that over the 16 x k winners: its picks are the block's top-k,
// best first.  ~20 us, against 35-50 us for sorting the few hundred survivors these stages see.
constexpr int kSelThreads = 1024;
constexpr int kSelPer = 8;
constexpr int kSelWaves = kSelThreads / 64;
#ifndef FSGPU_SEL_MIN_WAVES
#define FSGPU_SEL_MIN_WAVES 8
#endif
constexpr int kSelMinWaves = FSGPU_SEL_MIN_WAVES;   // waves per SIMD the unsorted selection is compiled for (8: two blocks per CU, 64 registers)

// One pass of the per-wave extraction: dst[0..k) <- the wave's k best among e[] and prev[0..k) (its earlier winners).
// KL = ceil(KMAX / 64): how many of the previous winners each lane carries.
template <int PER, int KL>
__device__ __forceinline__ void wave_select_pass(const u64 (&e)[PER], int k, const u64* prev, u64* dst, int lane) {
    u64 ee[PER + KL], key[PER + KL];
#pragma unroll
    for (int x = 0; x < PER; ++x) ee[x] = e[x];
#pragma unroll
    for (int c = 0; c < KL; ++c) ee[PER + c] = (prev && lane + 64 * c < k) ? prev[lane + 64 * c] : kEmpty;
#pragma unroll
    for (int x = 0; x < PER + KL; ++x) key[x] = ee[x] != kEmpty ? sortkey(ee[x]) : 0ull;
#pragma unroll
    for (int c = 0; c < KL; ++c)
        if (lane + 64 * c < k) dst[lane + 64 * c] = kEmpty;
    wave_lds_fence();
    wave_extract_topk<PER + KL>(key, ee, k, dst);
    wave_lds_fence();
}

// top[0..k) <- the k best of the 16 waves' winner lists win[wave * k + j], best first (kEmpty padded).  Wave 0 only.
// E = winners a lane holds (16 k <= 64 E): the rounds cost ~6 E + 36 instructions each and run on ONE wave — the serial
// tail of every selection — so the usual small ranks (k <= 16: 160 winners) take E = 4 instead of the general 16.
template <int E>
__device__ __forceinline__ void merge_wave_winners_e(const u64* win, int k, u64* top, int lane) {
    constexpr int NW = kSelWaves;
    u64 e2[E], key2[E];
#pragma unroll
    for (int x = 0; x < E; ++x) {
        const int i = lane + x * 64;
        e2[x] = i < NW * k ? win[i] : kEmpty;
        key2[x] = e2[x] != kEmpty ? sortkey(e2[x]) : 0ull;
    }
    top[lane] = kEmpty;
    wave_lds_fence();
    wave_extract_topk<E>(key2, e2, k, top);
    wave_lds_fence();
}
template <int KL>
__device__ __forceinline__ void merge_wave_winners(const u64* win, int k, u64* top, int lane) {
    static_assert(KL == 1, "ranks up to 64");
    if (k <= 16) merge_wave_winners_e<4>(win, k, top, lane);
    else if (k <= 32) merge_wave_winners_e<8>(win, k, top, lane);
    else merge_wave_winners_e<kSelWaves>(win, k, top, lane);
}

// SORTED = false: the extraction scheme above; its cost grows with k^2 (k rounds over lists that grow with k), fine up
// to k ~ 32.  SORTED = true (larger k: the int8 fast tier anchors on 3 x 30 = 90 candidates): the non-empty entries
// are compacted into LDS and bitonic-sorted by the whole block; top-k, threshold and candidate prefix fall out.
constexpr int kSelSortCap = 8192;   // live entries the sorted variant holds (dynamic LDS: 64 KB)
constexpr int kRescoreBatch = 6;    // slab loads of a candidate row in flight at a time (a row of 384 dimensions: two round trips; 4: -1 % of a step, 12: spills, -2.5 %)
constexpr int kSelQueryLds = 1024;  // dimensions of the re-score's query kept in LDS (longer queries are read in place)
constexpr int kRescoreBatchF32 = 3; // ... of an F32 row: a group is two 16-byte loads per lane, so 3 keep the same 24 registers in flight
#ifdef FSGPU_EXPERIMENTS
#define SEL_STAMP(slot)                                                                                            \
    do {                                                                                                             \
        if (args.stamps && (blockIdx.x & 255) == 0 && blockIdx.x < 1024 && threadIdx.x == 0)                    \
            args.stamps[(blockIdx.x >> 8) * 16 + (slot)] = (unsigned long long)clock64();                              \
    } while (0)
#else
#define SEL_STAMP(slot) \
    do {                \
    } while (0)
#endif
// F32 = the slab holds raw f32 rows (Quantization::F32): the finish re-scores in dot_product_f32_bytes_f32's order (quad_dot_f32,
// scan_common.hpp) instead of dot_product_f16_bytes_f32's; nothing else differs, and the F16 instantiations are the code they were.
template <bool FINISH, bool SORTED, bool F32 = false>
__global__ __launch_bounds__(kSelThreads, SORTED ? 4 : kSelMinWaves) void select_kernel(SelectArgs args) {
    static_assert(FINISH || !F32, "only the re-score reads the slab");
    constexpr int NT = kSelThreads, PER = kSelPer, NW = kSelWaves, POOL = (int)kSelectPool, KL = 1;
    static_assert(POOL == NT, "one pool entry per thread in the final selection");
    __shared__ u64 win[2][NW * 64 * KL];  // per-wave winners [wave][rank], ping-pong across passes
    __shared__ u64 top[64 * KL];          // block top-k, best first (extraction scheme)
    extern __shared__ __attribute__((aligned(16))) unsigned char sel_dyn[];
    u64* sbuf = reinterpret_cast<u64*>(sel_dyn);  // [kSelSortCap] in the sorted variant, unused otherwise
    __shared__ u64 pool[POOL];       // candidates (finish step: replaced by their exact entries)
    __shared__ int s_count;
    __shared__ float s_tau;
    __shared__ u64 s_gmax[64];
    __shared__ __attribute__((aligned(16))) float s_q[FINISH ? kSelQueryLds : 4];
    __shared__ int s_quick;
    __shared__ u64 s_kth[2];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    SEL_STAMP(0);
    if (args.big_pool && args.pool_flag && args.pool_flag[q] == 0) return;   // second chance: only the queries the first finish flagged
    // (called where every thread is past the barriers behind its read of the spill count)
    auto reset_spill = [&]() {
        if (tid == 0 && args.spill_reset) args.spill_reset[(size_t)q * kMfmaSpillCountStride] = 0u;
    };
    const int k = (int)args.k;
    // Everything the block needs first is REQUESTED first, in one round trip: the list lengths, the entries of the lists' first four
    // slots (speculatively — most lists hold fewer than four; what lies beyond a list's length is masked once the lengths are in), the
    // spill count, delta, the re-score's query.  (They used to be four dependent round trips: delta -> query -> lengths -> entries.)
    const u64* in = args.lists + (size_t)q * args.q_stride;
    const uint32_t* cnts = args.list_counts ? args.list_counts + (size_t)q * args.nlists : nullptr;
    constexpr uint32_t kSelCntCap = 512;
    constexpr uint32_t kSpecSlots = 4;
    __shared__ uint32_t s_cnt[kSelCntCap];   // the query's list lengths: one coalesced read instead of a dependent one per slot
    const uint32_t lists32 = args.nlists * args.list_len;
    uint32_t my_cnt = 0;
    if (cnts && (uint32_t)tid < args.nlists && (uint32_t)tid < kSelCntCap) my_cnt = cnts[tid];
    u64 e[PER];
    const bool spec = cnts != nullptr && !SORTED;
    if (spec) {
#pragma unroll
        for (int x = 0; x < PER; ++x) {
            const uint32_t i = tid + x * NT;
            e[x] = kEmpty;
            if (i < lists32) {
                const uint32_t l = i / args.list_len, j = i - l * args.list_len;
                if (j < kSpecSlots) e[x] = in[(size_t)l * args.l_stride + j];
            }
        }
    }
    uint32_t nspill = 0;
    if (args.spill) nspill = args.spill_count[(size_t)q * kMfmaSpillCountStride];
    const float dq = args.delta[q];
    float qreg[(kSelQueryLds + NT - 1) / NT];
    // (the padding slots of a round's last group lie past the end of the caller's query array: valid_queries bounds the read)
    const bool stage_q = FINISH && args.queries && (int)args.dim <= kSelQueryLds && (args.valid_queries == 0 || (uint32_t)q < args.valid_queries);
    if constexpr (FINISH) {
        if (stage_q) {
            const float* qsrc = args.queries + (size_t)q * (args.query_stride ? args.query_stride : args.dim);
#pragma unroll
            for (int x = 0; x < (kSelQueryLds + NT - 1) / NT; ++x) qreg[x] = tid + x * NT < (int)args.dim ? qsrc[tid + x * NT] : 0.f;
        }
    }
    if (cnts) {
        if ((uint32_t)tid < args.nlists && (uint32_t)tid < kSelCntCap) s_cnt[tid] = my_cnt;
        for (uint32_t i = tid + NT; i < args.nlists && i < kSelCntCap; i += NT) s_cnt[i] = cnts[i];
    }
    if constexpr (FINISH) {
        // the query of the exact re-score, parked in LDS (read by every candidate's quad); visible after the barriers below
        if (stage_q) {
#pragma unroll
            for (int x = 0; x < (kSelQueryLds + NT - 1) / NT; ++x)
                if (tid + x * NT < (int)args.dim) s_q[tid + x * NT] = qreg[x];
        }
    }
    if (cnts) __syncthreads();
    const uint32_t extra_end = lists32 + args.extra_len;
    nspill = nspill < args.spill_cap ? nspill : args.spill_cap;
    const uint32_t total32 = extra_end + nspill;
    const int npass = total32 ? (int)((total32 + NT * PER - 1) / (NT * PER)) : 1;
    // first = the first load of pass 0 after the speculative requests above: slots below kSpecSlots are already in e
    auto load_pass = [&](int p, u64 (&e)[PER], bool first = false) {
#pragma unroll
        for (int x = 0; x < PER; ++x) {
            const uint32_t i = (uint32_t)p * (NT * PER) + tid + x * NT;
            const bool have = first && spec && p == 0;
            if (!have) e[x] = kEmpty;
            if (i < lists32) {
                // (list lengths, staged in LDS above: only the slots that hold an entry are read — a few percent of them)
                const uint32_t l = i / args.list_len, j = i - l * args.list_len;
                const bool in_list = !cnts || j < (l < kSelCntCap ? s_cnt[l] : cnts[l]);
                if (have && j < kSpecSlots) {
                    if (!in_list) e[x] = kEmpty;
                } else if (in_list) {
                    e[x] = in[(size_t)l * args.l_stride + j];
                } else {
                    e[x] = kEmpty;
                }
            } else if (i < extra_end) {
                e[x] = args.extra[(size_t)q * args.extra_len + (i - lists32)];
            } else if (i < total32) {
                e[x] = args.spill[(size_t)q * args.spill_cap + (i - extra_end)];
            } else {
                e[x] = kEmpty;
            }
        }
    };
    if (tid == 0) s_count = 0;
    pool[tid] = kEmpty;
    int ncand = 0;
    if constexpr (SORTED) {
        __syncthreads();
        for (int p = 0; p < npass; ++p) {  // block-uniform
            load_pass(p, e);
#pragma unroll
            for (int x = 0; x < PER; ++x) {
                const bool ok = e[x] != kEmpty;
                const u64 m = __ballot(ok);
                if (m) {
                    int wbase = 0;
                    if (lane == 0) wbase = atomicAdd(&s_count, (int)__popcll(m));
                    wbase = __shfl(wbase, 0);
                    const int pos = wbase + (int)__popcll(m & ((1ull << lane) - 1ull));
                    if (ok && pos < kSelSortCap) sbuf[pos] = e[x];
                }
            }
        }
        __syncthreads();
        int cnt = s_count;
        if (cnt > kSelSortCap) {  // more live entries than the sort holds: the per-query path answers this one
            if (tid == 0 && args.overflow) args.overflow[q] = 1;
            cnt = kSelSortCap;
        }
        int np2 = 64;
        while (np2 < cnt) np2 <<= 1;
        for (int j = cnt + tid; j < np2; j += NT) sbuf[j] = kEmpty;
        block_sort_desc_rt<NT>(sbuf, np2, tid);
        if (tid == 0) {
            const float d = args.delta[q];
            float t = -INFINITY;   // fewer than k entries: everything is a candidate
            if (d < 0.f) {
                t = INFINITY;      // skipped query (padding / zero / non-finite): the exact path answers it
                if (args.overflow) args.overflow[q] = 1;
            } else if (k <= cnt) {
                t = __uint_as_float((uint32_t)(sbuf[k - 1] >> 32)) - 2.0f * d;
                if (!(t == t)) t = -INFINITY;
            } else if (args.tau_floor_in) {
                t = args.tau_floor_in[q];
            }
            s_tau = t;
            s_count = 0;
            if (args.tau_floor_out) args.tau_floor_out[q] = t;
            if (args.heur_rank && d >= 0.f && (int)args.heur_rank <= cnt) {
                const float th = __uint_as_float((uint32_t)(sbuf[args.heur_rank - 1] >> 32));
                if (th == th && th > t) t = th;
            }
            if (args.tau_out) args.tau_out[q] = t;
        }
        __syncthreads();
        if (!FINISH && !args.pool_out && !args.cand_counts) {
            reset_spill();
            return;
        }
        const float tau = s_tau;
        if (args.take_topk) {
            ncand = cnt < k ? cnt : k;  // exact scores: the candidates are the k best entries themselves
        } else {
            // sorted by (score desc, row asc): the entries at or above tau are a prefix
            for (int j = tid; j < cnt; j += NT)
                if (__uint_as_float((uint32_t)(sbuf[j] >> 32)) >= tau) atomicMax(&s_count, j + 1);
            __syncthreads();
            ncand = s_count;
            if (tau == -INFINITY && ncand > 0) {   // block-uniform; only a query without a threshold comes here
                // The entries that rank as -inf are ordered by row alone, so a NaN score can sit in front of a -inf one, inside the
                // prefix: it is no candidate (score >= tau is false for it, as in the extraction form) — close the gaps.  What lies
                // behind the candidates is not read again.
                __syncthreads();   // (every thread has read s_count)
                if (tid == 0) {
                    int f = ncand;
                    while (f > 0 && score_ord((uint32_t)(sbuf[f - 1] >> 32)) == score_ord(0xff800000u)) --f;
                    int w = f;
                    for (int j = f; j < ncand; ++j) {
                        const u64 v = sbuf[j];
                        const float s = __uint_as_float((uint32_t)(v >> 32));
                        if (s == s) sbuf[w++] = v;
                    }
                    s_count = w;
                }
                __syncthreads();
                ncand = s_count;
            }
        }
        pool[tid] = tid < ncand && tid < kSelSortCap ? sbuf[tid] : kEmpty;
        __syncthreads();
    } else {
        SEL_STAMP(1);
        // The threshold only has to lie AT OR BELOW (k-th best approximate score) - 2 delta: any k distinct entries bound the
        // k-th best from below.  In a selection that re-scores its candidates exactly (FINISH) and needs neither the exact top-k
        // of the approximate scores (take_topk) nor a rank of them (heur_rank), the k-th largest of the maxima of 64 interleaved
        // groups of the entries serves: ~9 k cycles instead of the ~30 k of the extraction rounds + the one-wave merge of their
        // winners (lab stamps, scripts/r03/select_lab.sh: 80 k -> ~55 k cycles per query block together with the re-score's
        // batched loads), at the price of a few more candidates for the exact re-score.  Selections whose threshold GATES a scan
        // (the sample stages without an exact anchor) keep the exact rank: a looser gate there costs the append-bound sample
        // pass more than the selection saves (measured: +0.11 ms per 1,024 queries).
        // (... and the first sample's selection of a wide round, whose only products are the proven floor and the HEURISTIC gate of
        // the anchoring-only second sample: the gate's rank taken among the group maxima sits a fraction of a rank lower)
        const bool gate_only = !FINISH && args.heur_rank != 0 && (int)args.heur_rank <= k && !args.pool_out && !args.cand_counts;
        const bool quick_bound = !args.take_topk && npass == 1 && k <= 32 && (FINISH ? args.heur_rank == 0 : gate_only);
        bool quick_ok = false;
        if (quick_bound) {
            load_pass(0, e, true);
            SEL_STAMP(2);
            // 64 groups along the diagonals of the (list, slot) grid — thread (list mod 64, slot) feeds group (list + slot) mod 64:
            // every group draws on all lists' heads evenly (lists fill from slot 0), and the entries of ONE list — a cluster's
            // best rows sit together in one block's list — land in different groups, so a topical corpus does not collapse the bound
            if (tid < 64) s_gmax[tid] = 0ull;
            u64 h = 0;
#pragma unroll
            for (int x = 0; x < PER; ++x) {
                const u64 key = e[x] != kEmpty ? sortkey(e[x]) : 0ull;
                h = key > h ? key : h;
            }
            __syncthreads();
            if (h != 0) atomicMax(&s_gmax[((tid >> 4) + (tid & 15)) & 63], h);
            __syncthreads();
            if (wave == 0) {
                // rank of each of the 64 group maxima among them: every value visits every lane through a scalar register
                const u64 mine = s_gmax[lane];
                const uint32_t mlo = (uint32_t)mine, mhi = (uint32_t)(mine >> 32);
                int greater = 0;
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    const u64 v = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)mhi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)mlo, j);
                    greater += v > mine ? 1 : 0;
                }
                const bool enough = __popcll(__ballot(mine != 0)) >= k;
                if (lane == 0) s_quick = enough ? 1 : 0;
                // keys are unique: exactly one group maximum has each rank
                if (enough && mine != 0 && greater == k - 1) s_kth[0] = mine;
                if (enough && args.heur_rank && mine != 0 && greater == (int)args.heur_rank - 1) s_kth[1] = mine;
                wave_lds_fence();
                if (enough && lane == 0) {
                    float t;
                    if (dq < 0.f) {
                        t = INFINITY;      // skipped query (padding / zero / non-finite): the exact path answers it
                        if (args.overflow) args.overflow[q] = 1;
                    } else {
                        t = __uint_as_float(score_from_sortkey(s_kth[0])) - 2.0f * dq;
                        if (!(t == t)) t = -INFINITY;
                    }
                    s_tau = t;
                    if (args.tau_floor_out) args.tau_floor_out[q] = t;
                    // (the heuristic gate of an anchoring-only sample stage: the score at that rank WITHOUT a margin — here the
                    // rank among the group maxima, a few ranks lower in the whole list; the proven floor above keeps it honest)
                    if (args.heur_rank && dq >= 0.f) {
                        const float th = __uint_as_float(score_from_sortkey(s_kth[1]));
                        if (th == th && th > t) t = th;
                    }
                    if (args.tau_out) args.tau_out[q] = t;
                }
            }
            __syncthreads();
            quick_ok = s_quick != 0;
        }
        if (!quick_ok) {
        for (int p = 0; p < npass; ++p) {  // block-uniform
            if (!(quick_bound && p == 0)) load_pass(p, e, p == 0);
            if (p == 0) SEL_STAMP(2);
            wave_select_pass<PER, KL>(e, k, p ? win[(p - 1) & 1] + wave * k : nullptr, win[p & 1] + wave * k, lane);
        }
        __syncthreads();
        SEL_STAMP(3);
        }
        if (!quick_ok && wave == 0) {
            merge_wave_winners<KL>(win[(npass - 1) & 1], k, top, lane);
            if (lane == 0) {
                const float d = args.delta[q];
                float t = -INFINITY;   // fewer than k entries: everything is a candidate
                if (d < 0.f) {
                    t = INFINITY;      // skipped query (padding / zero / non-finite): the exact path answers it
                    if (args.overflow) args.overflow[q] = 1;
                } else if (top[k - 1] != kEmpty) {
                    t = __uint_as_float((uint32_t)(top[k - 1] >> 32)) - 2.0f * d;
                    if (!(t == t)) t = -INFINITY;
                } else if (args.tau_floor_in) {
                    t = args.tau_floor_in[q];
                }
                s_tau = t;
                if (args.tau_floor_out) args.tau_floor_out[q] = t;
                if (args.heur_rank && d >= 0.f && (int)args.heur_rank <= k && top[args.heur_rank - 1] != kEmpty) {
                    const float th = __uint_as_float((uint32_t)(top[args.heur_rank - 1] >> 32));
                    if (th == th && th > t) t = th;
                }
                if (args.tau_out) args.tau_out[q] = t;
            }
        }
        __syncthreads();
        SEL_STAMP(4);
        if (!FINISH && !args.pool_out && !args.cand_counts) {
            reset_spill();
            return;
        }
        const float tau = s_tau;
        for (int p = 0; p < npass; ++p) {
            if (npass > 1) load_pass(p, e);  // a single pass still has its entries in registers
#pragma unroll
            for (int x = 0; x < PER; ++x) {
                const bool ok = e[x] != kEmpty && __uint_as_float((uint32_t)(e[x] >> 32)) >= tau;
                const u64 m = __ballot(ok);
                if (m) {
                    int wbase = 0;
                    if (lane == 0) wbase = atomicAdd(&s_count, (int)__popcll(m));
                    wbase = __shfl(wbase, 0);
                    const int pos = wbase + (int)__popcll(m & ((1ull << lane) - 1ull));
                    if (ok && pos < POOL) pool[pos] = e[x];
                }
            }
        }
        __syncthreads();
        if (args.take_topk) {
            // exact scores (int8 pass 1): the candidates are precisely the block's k best entries under the reference
            // order, ties at the k-th score included only by row order — not everything at or above the k-th score
            pool[tid] = tid < k ? top[tid] : kEmpty;
            if (tid == 0) {
                int n = 0;
                while (n < k && top[n] != kEmpty) ++n;
                s_count = n;
            }
            __syncthreads();
        }
        ncand = s_count;
    }
    SEL_STAMP(5);
    // big pool (sorted variant's finish): the candidates stay in the sort buffer — up to kSelSortCap of them are re-scored
    // exactly instead of POOL (a tight cluster puts thousands of rows inside the int8 filter's margin)
    const bool big = FINISH && SORTED && args.big_pool != 0 && !args.take_topk;
    const int pool_cap = big ? kSelSortCap : POOL;
    if (tid == 0) {
        if (args.cand_counts) args.cand_counts[q] = (uint32_t)ncand;
        if (!big && args.pool_flag) args.pool_flag[q] = ncand > pool_cap ? 1u : 0u;   // ... the big-pool launch behind this one takes it
        else if (ncand > pool_cap && args.overflow) args.overflow[q] = 1;
    }
    if (args.pool_out) args.pool_out[(size_t)q * POOL + tid] = pool[tid];
    reset_spill();   // (threshold steps of either kind — a sample stage's selection with an exact anchor is a FINISH instantiation)
    if constexpr (FINISH) {
        if (args.cand_approx_out && args.take_topk && tid < k) args.cand_approx_out[(size_t)q * args.cand_out_stride + tid] = pool[tid];
        // exact-order re-score (dot_product_f16_bytes_f32 order, as gather_dot_kernel): one quad per candidate,
        // 256 candidates per sweep; the entry is replaced by its exact counterpart in place
        const int dim = (int)args.dim;
        const int a = tid & 3;
        const int nc = ncand < pool_cap ? ncand : pool_cap;
        u64* cbuf = big ? sbuf : pool;   // (big: sbuf[0, ncand) are the candidates, best approximate score first)
        const float* qv = dim <= kSelQueryLds ? s_q : args.queries + (size_t)q * (args.query_stride ? args.query_stride : (uint32_t)dim);
        const size_t row_pitch = args.row_stride ? (size_t)args.row_stride : (size_t)dim * (F32 ? 4 : 2);
        const int chunks = dim >> 3, groups = chunks >> 2, leftover = chunks & 3;
        for (int c0 = 0; c0 < nc; c0 += NT / 4) {  // block-uniform trip count
            const int c = c0 + (tid >> 2);
            const u64 mine_e = c < nc ? cbuf[c] : kEmpty;
            const uint32_t grow = (uint32_t)mine_e;
            uint32_t row = grow - args.row_base;
            const bool mine = mine_e != kEmpty && row < args.nrows;
            if (!mine) row = 0;
            if constexpr (F32) {
                // (dense 16-byte aligned rows: launch_select checks dim % 8 and the row stride)
                const float* w = reinterpret_cast<const float*>(reinterpret_cast<const unsigned char*>(args.slab) + (size_t)row * row_pitch);
                const float sc = quad_dot_f32<kRescoreBatchF32>(w, qv, dim, a, true, args.hreduce);
                if (a == 0 && c < nc) cbuf[c] = mine ? pack(sc, grow) : kEmpty;
                continue;
            }
            const u32x4* p = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(args.slab) + (size_t)row * row_pitch);
            float acc[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[j] = 0.f;
            // (kRescoreBatch groups' slab loads in flight at a time: the loop was one HBM round trip per group — 12 for 384 dimensions,
            // ~20 k cycles of the finish's 80 k; the query's chunks come from LDS.  64 VGPRs per thread at this block size.)
            for (int g0 = 0; g0 < groups; g0 += kRescoreBatch) {
                u32x4 w[kRescoreBatch];
#pragma unroll
                for (int j = 0; j < kRescoreBatch; ++j)
                    if (g0 + j < groups) w[j] = p[4 * (g0 + j) + a];
#pragma unroll
                for (int j = 0; j < kRescoreBatch; ++j)
                    if (g0 + j < groups) {
                        const float4* qp = reinterpret_cast<const float4*>(qv + 32 * (g0 + j) + 8 * a);
                        chunk_mac(acc, w[j], qp[0], qp[1]);
                    }
            }
            if (a == 0)
                for (int ch = 4 * groups; ch < 4 * groups + leftover; ++ch) {
                    const u32x4 w = p[ch];
                    const float4* qp = reinterpret_cast<const float4*>(qv + 8 * ch);
                    chunk_mac(acc, w, qp[0], qp[1]);
                }
            const float sc = quad_finish(acc, args.hreduce);
            if (a == 0 && c < nc) cbuf[c] = mine ? pack(sc, grow) : kEmpty;  // only this quad touches its entry
        }
        __syncthreads();
        SEL_STAMP(6);
        if (args.stamps && (blockIdx.x & 255) == 0 && blockIdx.x < 1024 && threadIdx.x == 0) args.stamps[(blockIdx.x >> 8) * 16 + 15] = (unsigned long long)nc;
        if (args.cand_exact_out && args.take_topk && tid < k) args.cand_exact_out[(size_t)q * args.cand_out_stride + tid] = pool[tid];
        const int ko = (int)args.k_out;
        if (big) {
            // the exact entries, sorted again: the first k_out are the answer
            int np = 64;
            while (np < nc) np <<= 1;
            for (int j = nc + tid; j < np; j += NT) sbuf[j] = kEmpty;
            block_sort_desc_rt<NT>(sbuf, np, tid);
            if (tid < 64) top[tid] = tid < ko && tid < np ? sbuf[tid] : kEmpty;
        } else if (nc <= 64) {
            // the usual case (a few dozen candidates, all in pool[0, 64)): wave 0's picks ARE the block's top-k
            // (by rank: every key visits every lane through a scalar register; keys are unique, so the ranks are a permutation)
            if (wave == 0) {
                const u64 mine_e = pool[lane];
                const u64 mine = mine_e != kEmpty ? sortkey(mine_e) : 0ull;
                const uint32_t mlo = (uint32_t)mine, mhi = (uint32_t)(mine >> 32);
                int greater = 0;
#pragma unroll 8
                for (int j = 0; j < 64; ++j) {
                    const u64 v = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)mhi, j) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)mlo, j);
                    greater += v > mine ? 1 : 0;
                }
                top[lane] = kEmpty;
                wave_lds_fence();
                if (mine != 0 && greater < ko) top[greater] = mine_e;
                wave_lds_fence();
            }
        } else if (nc <= 256) {
            // up to 256 candidates: the same by four waves, the keys broadcast from LDS (the winners' buffer is free here)
            u64* keys = win[0];
            const u64 mine_e = tid < 256 ? pool[tid] : kEmpty;
            const u64 mine = mine_e != kEmpty ? sortkey(mine_e) : 0ull;
            if (tid < 256) keys[tid] = mine;
            if (tid < 64) top[tid] = kEmpty;
            __syncthreads();
            if (tid < 256 && mine != 0) {
                int greater = 0;
                const int nj = (nc + 7) & ~7;   // (the candidates are pool[0, nc))
#pragma unroll 8
                for (int j = 0; j < nj; ++j) greater += keys[j] > mine ? 1 : 0;
                if (greater < ko) top[greater] = mine_e;
            }
        } else {
            u64 e3[1];
            e3[0] = pool[tid];
            wave_select_pass<1, 1>(e3, ko, nullptr, win[0] + wave * ko, lane);
        }
        __syncthreads();
        SEL_STAMP(7);
        if (wave == 0) {
            if (!big && nc > 256) merge_wave_winners<1>(win[0], ko, top, lane);
            if (args.anchor_unit && args.tau_out && lane == 0) {
                // the k-th best exact score among real rows is a lower bound on the final k-th best; in filter units, minus one
                // delta (and the rounding of the product), it bounds every true top-k row's approximate score from below
                const float d = args.delta[q];
                const u64 kth = top[ko - 1];
                float t = s_tau;
                if (d >= 0.f && kth != kEmpty) {
                    const float sk = __uint_as_float((uint32_t)(kth >> 32));
                    const float v = sk * args.anchor_unit[q];
                    const float te = v - d - fabsf(v) * 1e-6f - 1.0f;
                    if (te == te && te > t) t = te;
                }
                args.tau_out[q] = t;
            }
            int n = 0;
            for (int j = lane; j < (int)args.out_stride; j += 64) {
                const u64 cnd = j < ko ? top[j] : kEmpty;
                if (args.out_rows) args.out_rows[(size_t)q * args.out_stride + j] = (uint32_t)cnd;
                if (args.out_scores) args.out_scores[(size_t)q * args.out_stride + j] = __uint_as_float((uint32_t)(cnd >> 32));
                if (args.out_packed) args.out_packed[(size_t)q * args.out_stride + j] = cnd;
                n += cnd != kEmpty ? 1 : 0;
            }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) n += __shfl_xor(n, off);
            if (lane == 0 && args.out_counts) args.out_counts[q] = (uint32_t)n;
        }
        SEL_STAMP(8);
    }
}

// max over rows of the f32 Euclidean norm (order-free upper bound use only), as float bits via atomic max.
__global__ __launch_bounds__(256) void max_row_norm_kernel(const unsigned short* __restrict__ slab, uint32_t nrows,
                                                           uint32_t dim, uint32_t row_stride_halves,
                                                           unsigned int* __restrict__ out_bits) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave_gid = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * 256) >> 6;
    float m = 0.f;
    for (uint32_t row = wave_gid; row < nrows; row += nwaves) {
        const _Float16* p = reinterpret_cast<const _Float16*>(slab) + (size_t)row * row_stride_halves;
        float s = 0.f;
        for (uint32_t i = lane; i < dim; i += 64) {
            const float v = (float)p[i];
            s += v * v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        m = fmaxf(m, s);
    }
    if (lane == 0) atomicMax(out_bits, __float_as_uint(sqrtf(m) * 1.0001f));
}

// ... over dense f32 rows (an F32 slab: only the rotation decision of its int8 filter copy reads it).
__global__ __launch_bounds__(256) void max_row_norm_f32_kernel(const float* __restrict__ rows, uint32_t nrows, uint32_t dim,
                                                               unsigned int* __restrict__ out_bits) {
    const int lane = threadIdx.x & 63;
    const uint32_t wave_gid = (blockIdx.x * 256 + threadIdx.x) >> 6;
    const uint32_t nwaves = (gridDim.x * 256) >> 6;
    float m = 0.f;
    for (uint32_t row = wave_gid; row < nrows; row += nwaves) {
        const float* p = rows + (size_t)row * dim;
        float s = 0.f;
        for (uint32_t i = lane; i < dim; i += 64) {
            const float v = p[i];
            s += v * v;
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
        m = fmaxf(m, s);
    }
    if (lane == 0) atomicMax(out_bits, __float_as_uint(sqrtf(m) * 1.0001f));
}

// f32 queries -> zero-padded f16 rows + the per-query error bound delta_q (see header).
__global__ __launch_bounds__(256) void prepare_queries_kernel(const float* __restrict__ q, uint32_t nq, uint32_t q_stride,
                                                              uint32_t dim, const unsigned int* __restrict__ max_norm_bits,
                                                              _Float16* __restrict__ qh, float* __restrict__ delta) {
    __shared__ float red[4];
    __shared__ int unrepresentable;
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) unrepresentable = 0;
    __syncthreads();
    float s = 0.f;
    bool bad = false;
    for (uint32_t i = tid; i < dim; i += 256) {
        const float v = b < nq ? q[(size_t)b * q_stride + i] : 0.f;
        qh[(size_t)b * dim + i] = (_Float16)v;
        s += v * v;
        // |v| above the largest finite f16 (65504) rounds to +-inf (and NaN stays NaN): the approximate scores of such a
        // query are inf / NaN and the error bound says nothing about them — the exact kernels answer it
        bad |= !(fabsf(v) <= 65504.0f);
    }
    if (__any(bad) && lane == 0) unrepresentable = 1;
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (lane == 0) red[wave] = s;
    __syncthreads();
    if (tid == 0) {
        const float qnorm = sqrtf(red[0] + red[1] + red[2] + red[3]) * 1.0001f;
        const float mx = __uint_as_float(*max_norm_bits);
        const float rel = 4.8852e-4f /* 2^-11 (1 + 2^-11) */ + (float)dim * 1.1920929e-7f /* 2^-23 */;
        float d = rel * mx * qnorm + sqrtf((float)dim) * 2.9802322e-8f /* 2^-25 */ * mx;
        // padding rows, all-zero and non-finite queries cannot be certified: negative delta = "skip" marker
        if (b >= nq || !(qnorm > 0.f) || !__builtin_isfinite(d) || unrepresentable) d = -1.0f;
        delta[b] = d;
    }
}

// quantize_i8_query (search.rs:1616-1626) for a group of queries: per-query max-abs scale 127/max (f32::max ignores
// NaN), round half away from zero, clamp, NaN -> 0; an all-zero (or empty-max) query quantises to zeros.  Padding rows
// are zero and marked "skip" (delta < 0); real queries get delta = 0: the int8 scores are exact.
// (lim = 7, floor = 1e-9: the levels of pack_4bit_query, search.rs:1640-1653, one per byte — the batched 4-bit pass 1)
__global__ __launch_bounds__(256) void prepare_queries_i8_kernel(const float* __restrict__ q, uint32_t nq, uint32_t dim,
                                                                 signed char* __restrict__ qi8, float* __restrict__ delta,
                                                                 float lim, float floor) {
    __shared__ float red[4];
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    float m = 0.f;
    if (b < nq)
        for (uint32_t i = tid; i < dim; i += 256) m = fmaxf(m, fabsf(q[(size_t)b * dim + i]));
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) red[wave] = m;
    __syncthreads();
    const float max_abs = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    const bool zero = b >= nq || !(max_abs > floor);
    const float scale = zero ? 0.f : lim / max_abs;
    for (uint32_t i = tid; i < dim; i += 256) {
        signed char o = 0;
        if (!zero) {
            float v = roundf(q[(size_t)b * dim + i] * scale);
            if (v == v) o = (signed char)(int)fminf(fmaxf(v, -lim), lim);
        }
        qi8[(size_t)b * dim + i] = o;
    }
    if (tid == 0) delta[b] = b < nq ? 0.0f : -1.0f;
}

// The int8 FILTER of the exact search: the same query quantiser (per-query max-abs scale c_q = fl(127 / max), round half
// away from zero), but the integer scores are not the answer — they select the rows whose exact score is then computed
// in the reference's order, and delta_q is a PROVEN bound on how far an integer score can sit from the exact one.
//
// With the slab scale c_s (int8_kernels.hip: x_i = (r_i + eps_i) / c_s) and q_i = (p_i + eta_i) / c_q, the real-number dot
// is  S = (idot + sum eps_i p_i + sum r_i eta_i + sum eps_i eta_i) / (c_s c_q), so in units of the integer score
//     |idot - S c_s c_q| <= min(0.5' |p|_1, E2 |p|_2) + min(0.5' R1, H2 R2) + min(0.25' dim, E2 H2)
// (0.5' = 0.5 + the rounding of the scaled product; E2 / R1 / R2 = the slab's measured maxima over rows of |eps|_2, |r|_1,
// |r|_2; H2 = |eta|_2 measured here; Hoelder with (inf, 1) or Cauchy-Schwarz, whichever is smaller), and the reference's
// f32 score differs from S by at most dim 2^-23 |x|_2 |q|_2 + dim 2^-149 (rounded products and sums in ANY order; products
// may underflow), i.e. dim 2^-23 (R2 + E2)(P2 + H2) + dim 2^-149 c_s c_q in integer-score units.  c_s c_q > 0 is common to
// all rows of a query, so ranking by S c_s c_q is ranking by S, and the two-sided margin argument of the header applies
// verbatim with delta_q = that sum (inflated by 1e-3, + 1 for the f32 subtraction a_k - 2 delta; the integer scores convert
// to f32 exactly up to dim 1040).  Queries with an element that is not finite or above 65504 (an f32 product could
// overflow), zero queries, padding, and every query of a slab that holds a non-finite value or only zeros are marked
// "skip" (delta < 0): the f16 filter or the exact kernels answer them.
__global__ __launch_bounds__(256) void prepare_queries_i8_filter_kernel(const float* __restrict__ q, uint32_t nq, uint32_t q_stride,
                                                                        uint32_t dim, const unsigned int* __restrict__ slab_max_bits,
                                                                        const unsigned int* __restrict__ slab_stats,
                                                                        signed char* __restrict__ qi8, float* __restrict__ delta,
                                                                        float* __restrict__ unit_out, double extra_coeff) {
    __shared__ float redf[4];
    __shared__ unsigned int redu[2][4];
    __shared__ int s_bad;
    const uint32_t b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) s_bad = 0;
    float m = 0.f;
    bool bad = false;
    if (b < nq)
        for (uint32_t i = tid; i < dim; i += 256) {
            const float v = q[(size_t)b * q_stride + i];
            m = fmaxf(m, fabsf(v));
            bad |= !(fabsf(v) <= 65504.0f);
        }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    if (lane == 0) redf[wave] = m;
    __syncthreads();
    if (__any(bad) && lane == 0) s_bad = 1;
    const float max_abs = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    const bool zero = b >= nq || !(max_abs > 0.0f);
    const float scale = zero ? 0.f : 127.0f / max_abs;
    float h2 = 0.f;
    unsigned int p1 = 0, p2 = 0;
    for (uint32_t i = tid; i < dim; i += 256) {
        signed char o = 0;
        if (!zero) {
            const float y = q[(size_t)b * q_stride + i] * scale;
            float v = roundf(y);
            if (v == v) {
                v = fminf(fmaxf(v, -127.0f), 127.0f);
                o = (signed char)(int)v;
                const float e = fabsf(y - v) + 8e-6f;
                h2 += e * e;
            }
        }
        const int oi = (int)o;
        p1 += (unsigned int)(oi < 0 ? -oi : oi);
        p2 += (unsigned int)(oi * oi);
        qi8[(size_t)b * dim + i] = o;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        h2 += __shfl_xor(h2, off);
        p1 += __shfl_xor(p1, off);
        p2 += __shfl_xor(p2, off);
    }
    __syncthreads();  // everyone has read redf
    if (lane == 0) {
        redf[wave] = h2;
        redu[0][wave] = p1;
        redu[1][wave] = p2;
    }
    __syncthreads();
    if (tid == 0) {
        const double slab_max = (double)__uint_as_float(*slab_max_bits);
        const double E2 = sqrt((double)__uint_as_float(slab_stats[0])) * 1.001;
        const double R1 = (double)slab_stats[1];
        const double R2 = sqrt((double)slab_stats[2]);
        const bool slab_bad = slab_stats[3] != 0 || !(slab_max > 0.0) || !(slab_max <= 65504.0);
        const double H2 = sqrt((double)(redf[0] + redf[1] + redf[2] + redf[3])) * 1.001;
        const double P1 = (double)(redu[0][0] + redu[0][1] + redu[0][2] + redu[0][3]);
        const double P2 = sqrt((double)(redu[1][0] + redu[1][1] + redu[1][2] + redu[1][3]));
        const double n = (double)dim;
        const double c_s = 127.0 / slab_max * 1.000001, c_q = (double)scale * 1.000001;
        double d = fmin(0.50001 * P1, E2 * P2) + fmin(0.50001 * R1, H2 * R2) + fmin(0.25001 * n, E2 * H2);
        // (extra_coeff: what a ROTATED filter copy adds — slab and queries went through an orthogonal map in f64 and were rounded once
        // to f32: |x . q - x' . q'| <= (|R^T R - I| + 2.01 x 2^-24) |x| |q|, in the same units as the f32-accumulation term beside it)
        d += (n * 1.1920929e-7 /* 2^-23 */ + extra_coeff) * (R2 + E2) * (P2 + H2) + n * 1.5e-45 /* > 2^-149 */ * c_s * c_q;
        d = d * 1.001 + 1.0;
        float out = (float)d;
        if (!((double)out >= d)) out = __uint_as_float(__float_as_uint(out) + 1u);  // round up
        if (zero || s_bad || slab_bad || dim > 1040u || !__builtin_isfinite(out) || !(out < 1.0e9f)) out = -1.0f;
        delta[b] = out;
        // integer-score units per exact-score unit, for thresholds anchored on exact scores (select_kernel, anchor_unit)
        if (unit_out) unit_out[b] = out < 0.f ? 0.f : (127.0f / __uint_as_float(*slab_max_bits)) * scale;
    }
}

// ---- launchers ----------------------------------------------------------------------------------------------

static std::atomic<const char*> g_last_main_pass_kernel{""};
const char* last_main_pass_kernel() { return g_last_main_pass_kernel.load(std::memory_order_relaxed); }
void note_main_pass_kernel(const char* name) { g_last_main_pass_kernel.store(name, std::memory_order_relaxed); }

bool scan_mfma_supported(int dim) { return dim == 64 || dim == 128 || dim == 256 || dim == 384; }

template <int DIM, int NQT, int WPB, int STAGE, int RT, bool PF, int EB>
static hipError_t launch_mfma_s(const MfmaScanArgs& args, int grid, hipStream_t stream, int* occupancy) {
    // candidate staging: 32 slots per (query, block), 16 for the 160-query shape (the query tile takes 128 KB there)
    constexpr size_t kSlots = NQT > 8 ? 16 : kMfmaMaxSlots;
    const size_t lds = (size_t)NQT * 16 * (DIM * EB + 32) + (STAGE ? (size_t)NQT * 16 * (4 + 8 * kSlots) : 0);
    auto kern = scan_mfma_kernel<DIM, NQT, WPB, STAGE, RT, PF, EB>;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    if (occupancy) {
        int blocks = 0;
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, kern, WPB * 64, lds) != hipSuccess || blocks < 1) blocks = 1;
        *occupancy = blocks;
        return hipSuccess;
    }
    if (STAGE == 2) {
        // the instantiation the main pass runs, spelled as rocprofv3 prints it: bench.py matches a committed PMC summary
        // against it and refuses a figure that belongs to another kernel
        static const std::string name = "scan_mfma_kernel<" + std::to_string(DIM) + ", " + std::to_string(NQT) + ", " +
                                        std::to_string(WPB) + ", " + std::to_string(STAGE) + ", " + std::to_string(RT) + ", " +
                                        (PF ? "true" : "false") + ", " + std::to_string(EB) + ">";
        g_last_main_pass_kernel.store(name.c_str(), std::memory_order_relaxed);
    }
    hipLaunchKernelGGL(kern, dim3(grid, args.groups ? args.groups : 1), dim3(WPB * 64), lds, stream, args);
    return hipGetLastError();
}

template <int DIM, int NQT, int WPB, int RT, bool PF, int EB>
static hipError_t launch_mfma_t(const MfmaScanArgs& args, int grid, hipStream_t stream, int* occupancy) {
    if (args.stage == 0) return launch_mfma_s<DIM, NQT, WPB, 0, 1, true, EB>(args, grid, stream, occupancy);
    if (args.stage == 1) return launch_mfma_s<DIM, NQT, WPB, 1, RT, PF, EB>(args, grid, stream, occupancy);
    return launch_mfma_s<DIM, NQT, WPB, 2, RT, PF, EB>(args, grid, stream, occupancy);
}

// Shapes (nqt = query tiles of 16; wpb = waves per block; rt = 16-row sub-tiles per wave iteration):
//   shape 0: nqt 4, wpb 4, rt 1, register double buffer   (64 queries)
//   shape 1: nqt 8, wpb 8, rt 1, register double buffer   (128 queries, 100 KB LDS -> one block per CU)
//   shape 2: nqt 8, wpb 8, rt 2, single buffer            (128 queries, half the LDS reads per row)
//   shape 3: nqt 8, wpb 4, rt 2, register double buffer   (one wave per SIMD, 512 registers)
//   shape 4: nqt 8, wpb 8, rt 4, single buffer            (int8 only: 64-row tiles = the same 24 KB per wave as shape 2 on f16)
//   shape 5: nqt 10, wpb 8, rt 2, single buffer           (160 queries: 128 KB of LDS for the query tile)
int scan_mfma_waves_per_block(int shape) { return shape == 0 || shape == 3 ? 4 : 8; }
int scan_mfma_rows_per_tile(int shape) { return shape == 4 ? 64 : (shape >= 2 ? 32 : 16); }  // shape 5: 32
int scan_mfma_query_tiles(int shape) { return shape == 0 ? 4 : (shape == 5 ? 10 : 8); }
int scan_mfma_max_slots(int shape) { return shape == 5 ? 16 : (int)kMfmaMaxSlots; }
bool scan_mfma_shape_built(int shape) {   // (the cases of launch_mfma_d)
#ifdef FSGPU_EXPERIMENTS
    return shape >= 0 && shape <= 5;
#else
    return shape == 0 || shape == 2;
#endif
}
int scan_mfma_planner_shape(int requested, int elem_bytes) {
    const int last = elem_bytes == 1 ? 4 : 3;   // (shape 4 is int8 only; 0 and 5 are the planner's own choices, not a request's)
    return requested >= 1 && requested <= last && scan_mfma_shape_built(requested) ? requested : 2;
}

template <int DIM, int EB>
static hipError_t launch_mfma_d(const MfmaScanArgs& args, int shape, int grid, hipStream_t stream, int* occupancy) {
    switch (shape) {
        case 0: return launch_mfma_t<DIM, 4, 4, 1, true, EB>(args, grid, stream, occupancy);
        case 2: return launch_mfma_t<DIM, 8, 8, 2, false, EB>(args, grid, stream, occupancy);
#ifdef FSGPU_EXPERIMENTS
        // the shapes the planner no longer picks (measured and dropped: HISTORY.md, profiles/r06/lds_query_shape_ab.txt) — shapes 4 and 5
        // spill in their main-pass instantiations, so they are not even compiled into the shipped library
        case 1: return launch_mfma_t<DIM, 8, 8, 1, true, EB>(args, grid, stream, occupancy);
        case 3: return launch_mfma_t<DIM, 8, 4, 2, true, EB>(args, grid, stream, occupancy);
        case 4:
            if constexpr (EB == 1) return launch_mfma_t<DIM, 8, 8, 4, false, EB>(args, grid, stream, occupancy);
            return hipErrorInvalidValue;
        case 5: return launch_mfma_t<DIM, 10, 8, 2, false, EB>(args, grid, stream, occupancy);
#endif
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_scan_mfma(const MfmaScanArgs& args, int shape, int grid, hipStream_t stream, int* occupancy) {
    if (args.elem_bytes == 1) {
        switch (args.dim) {
            case 64: return launch_mfma_d<64, 1>(args, shape, grid, stream, occupancy);
            case 128: return launch_mfma_d<128, 1>(args, shape, grid, stream, occupancy);
            case 256: return launch_mfma_d<256, 1>(args, shape, grid, stream, occupancy);
            case 384: return launch_mfma_d<384, 1>(args, shape, grid, stream, occupancy);
            default: return hipErrorInvalidValue;
        }
    }
    switch (args.dim) {
        case 64: return launch_mfma_d<64, 2>(args, shape, grid, stream, occupancy);
        case 128: return launch_mfma_d<128, 2>(args, shape, grid, stream, occupancy);
        case 256: return launch_mfma_d<256, 2>(args, shape, grid, stream, occupancy);
        case 384: return launch_mfma_d<384, 2>(args, shape, grid, stream, occupancy);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_prepare_queries_i8(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, void* qi8, float* delta,
                                     hipStream_t stream, int bits) {
    hipLaunchKernelGGL(prepare_queries_i8_kernel, dim3(nq_pad), dim3(256), 0, stream, q, nq, dim,
                       static_cast<signed char*>(qi8), delta, bits == 4 ? 7.0f : 127.0f, bits == 4 ? 1e-9f : 0.0f);
    return hipGetLastError();
}

hipError_t launch_prepare_queries_i8_filter(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t q_stride,
                                            const unsigned int* slab_max_bits, const unsigned int* slab_stats, void* qi8,
                                            float* delta, hipStream_t stream, float* unit_out, double extra_coeff) {
    hipLaunchKernelGGL(prepare_queries_i8_filter_kernel, dim3(nq_pad), dim3(256), 0, stream, q, nq, q_stride ? q_stride : dim, dim,
                       slab_max_bits, slab_stats, static_cast<signed char*>(qi8), delta, unit_out, extra_coeff);
    return hipGetLastError();
}

// Root of a row-sharded two-pass search: one block per query, up to 1,024 candidate pairs.
__global__ __launch_bounds__(256) void two_pass_merge_kernel(const u64* __restrict__ approx_lists, const u64* __restrict__ exact_lists,
                                                             uint32_t nshards, uint64_t shard_pitch, uint32_t nq, uint32_t cc, uint32_t k,
                                                             uint32_t out_stride,
                                                             uint32_t* __restrict__ out_rows, float* __restrict__ out_scores,
                                                             uint32_t* __restrict__ out_counts) {
    __shared__ u64 akey[1024];    // pass-1 sort keys, then the exact sort keys of the chosen candidates
    __shared__ u64 aval[1024];    // the exact entry that travels with each key
    const uint32_t q = blockIdx.x;
    const int tid = threadIdx.x;
    const uint32_t total = nshards * cc;   // <= 1024 (checked by the launcher)
    int np = 64;
    while ((uint32_t)np < total) np <<= 1;
    for (int i = tid; i < np; i += 256) {
        u64 ka = 0, ve = kEmpty;
        if ((uint32_t)i < total) {
            const uint32_t s = (uint32_t)i / cc, j = (uint32_t)i - s * cc;
            const u64 a = approx_lists[(size_t)s * shard_pitch + (size_t)q * cc + j];
            if (a != kEmpty) {
                ka = sortkey(a);
                ve = exact_lists[(size_t)s * shard_pitch + (size_t)q * cc + j];
            }
        }
        akey[i] = ka;
        aval[i] = ve;
    }
    __syncthreads();
    // bitonic sort by pass-1 key, descending (keys of real rows are distinct; empty slots have key 0 and sink)
    auto sort_pairs = [&](int n) {
        for (int size = 2; size <= n; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) {
                for (int i = tid; i < n / 2; i += 256) {
                    const int lo = (i / stride) * stride * 2 + (i % stride), hi = lo + stride;
                    const bool desc = ((lo & size) == 0);
                    const u64 x = akey[lo], y = akey[hi];
                    if ((x < y) == desc) {
                        akey[lo] = y;
                        akey[hi] = x;
                        const u64 t = aval[lo];
                        aval[lo] = aval[hi];
                        aval[hi] = t;
                    }
                }
                __syncthreads();
            }
    };
    sort_pairs(np);
    // the first cc entries are the corpus-wide pass-1 candidates: re-key them by their exact entries
    int np2 = 64;
    while ((uint32_t)np2 < cc) np2 <<= 1;
    for (int i = tid; i < np2; i += 256) {
        const bool real = (uint32_t)i < cc && akey[i] != 0 && aval[i] != kEmpty;
        const u64 v = real ? aval[i] : kEmpty;
        akey[i] = real ? sortkey(v) : 0;
        aval[i] = v;
    }
    __syncthreads();
    sort_pairs(np2);
    uint32_t n = 0;
    for (uint32_t j = (uint32_t)tid; j < out_stride; j += 256) {
        const u64 v = j < k && j < (uint32_t)np2 && akey[j] != 0 ? aval[j] : kEmpty;
        if (out_rows) out_rows[(size_t)q * out_stride + j] = (uint32_t)v;
        if (out_scores) out_scores[(size_t)q * out_stride + j] = __uint_as_float((uint32_t)(v >> 32));
    }
    if (tid == 0 && out_counts) {
        const uint32_t lim = k < (uint32_t)np2 ? k : (uint32_t)np2;
        while (n < lim && akey[n] != 0) ++n;
        out_counts[q] = n;
    }
}

bool two_pass_merge_args_ok(uint32_t nshards, uint32_t cc, uint32_t k) { return !(cc == 0 || (uint64_t)nshards * cc > 1024 || k > cc); }

hipError_t launch_two_pass_merge(const u64* approx_lists, const u64* exact_lists, uint32_t nshards, uint64_t shard_pitch, uint32_t nq,
                                 uint32_t cc, uint32_t k, uint32_t out_stride, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                 hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (!two_pass_merge_args_ok(nshards, cc, k)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(two_pass_merge_kernel, dim3(nq), dim3(256), 0, stream, approx_lists, exact_lists, nshards, shard_pitch, nq, cc, k,
                       out_stride, out_rows, out_scores, out_counts);
    return hipGetLastError();
}

// See GroupSelectArgs (kernels.hpp).  1,024 threads: one entry each -> every wave's PERW best -> wave 0 picks kGroupsTaken of those
// (RANK: the k best, k <= 64, and that is all) -> a quad per row of the taken groups (8 x 24 = 192 rows) re-scores it -> the k-th best
// by rank among the <= 256 exact entries.  PERW winners per wave: a small slab's sample fills only a few waves' worth of entries, and
// the rank form needs 64 of them (8 / 16: from 192 / 256 entries on the picks are complete unless one wave holds more than PERW of them).
// 512 threads (two entries each): four blocks per CU, i.e. all of a 1,024-query round resident at once — the kernel is a chain of
// dependent round trips per block, and with 1,024-thread blocks a round took two waves of blocks.
// Round 6: two sizes of each form.  M = 32 groups taken (256 rows re-scored) serves ranks up to 32 — the two-tier flow fetches
// k x candidate_multiplier = 30 per tier (rrf.rs:113-115) and used to fall back to the two thresholded sample stages for it (0.8 ms of a
// 3.6 ms step at 10M rows against 0.3); KCAP = 128 serves the int8 two-pass at 3 x 30 = 90 candidates (32 winners per wave: the top
// 90 of 1,024 entries put ~11 in a wave's 128 on average).
// F32: the rows are raw f32 (Quantization::F32) and are re-scored in dot_product_f32_bytes_f32's order, as in select_kernel.
template <bool RANK, int M, int KCAP, bool F32 = false>
__global__ __launch_bounds__(512) void select_groups_kernel(GroupSelectArgs args) {
    static_assert(!(RANK && F32), "the rank form reads no rows");
    constexpr int NT = 512, NW = NT / 64, PERT = 1024 / NT, PERW = RANK ? KCAP / 4 : 8, W0 = NW * PERW / 64, NR = M * 8;
    static_assert(NR <= 256 && NR <= NT && NW * PERW % 64 == 0 && W0 >= 1, "W0 winners per lane of wave 0; the rank loop runs on NR threads");
    static_assert(M <= 64 && KCAP >= 64 && KCAP % 64 == 0 && (RANK || M <= NW * PERW), "wave 0 picks M (or k <= KCAP) of the waves' winners");
    __shared__ u64 win[NW * PERW];
    __shared__ u64 top[KCAP];
    __shared__ u64 pool[256];
    __shared__ u64 keys[256];
    __shared__ __attribute__((aligned(16))) float s_q[kSelQueryLds];
    __shared__ u64 s_kth;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q = blockIdx.x;
    const int k = (int)args.k;
    const float d = args.delta[q];
    const bool real_query = args.valid_queries == 0 || (uint32_t)q < args.valid_queries;
    const int dim = (int)args.dim;
    if (real_query) {
        const float* qsrc = args.queries + (size_t)q * (args.query_stride ? args.query_stride : args.dim);
        for (int i = tid; i < dim && i < kSelQueryLds; i += NT) s_q[i] = qsrc[i];
    }
    u64 e[PERT], key[PERT];
#pragma unroll
    for (int x = 0; x < PERT; ++x) {
        const uint32_t i = (uint32_t)tid + (uint32_t)x * NT;
        e[x] = i < args.nentries ? args.groups[(size_t)q * args.nentries + i] : kEmpty;
        key[x] = e[x] != kEmpty ? sortkey(e[x]) : 0ull;
    }
    if (lane < PERW) win[wave * PERW + lane] = kEmpty;
    if (tid < 256) pool[tid] = kEmpty;
    if (tid == 0) s_kth = 0ull;
    wave_lds_fence();
    wave_extract_topk<PERT>(key, e, PERW, win + wave * PERW);
    __syncthreads();
    if (wave == 0) {
        u64 e2[W0], key2[W0];
#pragma unroll
        for (int x = 0; x < W0; ++x) {
            e2[x] = win[lane + 64 * x];
            key2[x] = e2[x] != kEmpty ? sortkey(e2[x]) : 0ull;
        }
#pragma unroll
        for (int x = 0; x < KCAP / 64; ++x) top[lane + 64 * x] = kEmpty;
        wave_lds_fence();
        wave_extract_topk<W0>(key2, e2, RANK ? (k < KCAP ? k : KCAP) : M, top);
        wave_lds_fence();
    }
    __syncthreads();
    if constexpr (RANK) {
        if (tid == 0) {
            float t = -INFINITY;   // fewer than k groups: everything is a candidate
            if (d < 0.f || !real_query) {
                t = INFINITY;
                if (args.overflow) args.overflow[q] = 1;
            } else if (k <= KCAP && top[k - 1] != kEmpty) {
                const float ta = __uint_as_float((uint32_t)(top[k - 1] >> 32)) - 2.0f * d;
                if (ta == ta) t = ta;
            }
            args.tau_out[q] = t;
            if (args.spill_reset) args.spill_reset[(size_t)q * kMfmaSpillCountStride] = 0u;
        }
        return;
    }
    // exact-order re-score (dot_product_f16_bytes_f32 order, as gather_dot_kernel and select_kernel's finish): a quad per row
    for (int c0 = 0; c0 < NR; c0 += NT / 4) {   // (block-uniform: NR / (NT / 4) sweeps of a quad per row)
        const int c = c0 + (tid >> 2), a = tid & 3;
        const int gi = c >> 3, pos = c & 7;
        const u64 ge = c < NR ? top[gi] : kEmpty;
        const uint32_t grow = (uint32_t)ge + (uint32_t)((pos >> 2) * 16 + (pos & 3));
        uint32_t row = grow - args.row_base;
        bool mine = real_query && ge != kEmpty && row < args.nrows && dim <= kSelQueryLds;
        if (mine && args.live) mine = ((args.live[row >> 6] >> (row & 63)) & 1ull) != 0;
        if (mine && args.allow) mine = ((args.allow[row >> 6] >> (row & 63)) & 1ull) != 0;
        // (every lane of a quad computes the same predicate: the quad shuffles below see whole quads)
        if (!mine) row = 0;
        if constexpr (F32) {
            const float* w = reinterpret_cast<const float*>(args.slab) + (size_t)row * (size_t)dim;
            const float sc = quad_dot_f32<kRescoreBatchF32>(w, s_q, dim, a, true, args.hreduce);
            if (a == 0 && c < NR && mine) pool[c] = pack(sc, grow);
            continue;
        }
        const u32x4* p = reinterpret_cast<const u32x4*>(reinterpret_cast<const unsigned char*>(args.slab) + (size_t)row * ((size_t)dim * 2));
        float acc[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j] = 0.f;
        const int chunks = dim >> 3, groups = chunks >> 2, leftover = chunks & 3;
        for (int g0 = 0; g0 < groups; g0 += kRescoreBatch) {
            u32x4 w[kRescoreBatch];
#pragma unroll
            for (int j = 0; j < kRescoreBatch; ++j)
                if (g0 + j < groups) w[j] = p[4 * (g0 + j) + a];
#pragma unroll
            for (int j = 0; j < kRescoreBatch; ++j)
                if (g0 + j < groups) {
                    const float4* qp = reinterpret_cast<const float4*>(s_q + 32 * (g0 + j) + 8 * a);
                    chunk_mac(acc, w[j], qp[0], qp[1]);
                }
        }
        if (a == 0)
            for (int ch = 4 * groups; ch < 4 * groups + leftover; ++ch) {
                const u32x4 w = p[ch];
                const float4* qp = reinterpret_cast<const float4*>(s_q + 8 * ch);
                chunk_mac(acc, w, qp[0], qp[1]);
            }
        const float sc = quad_finish(acc, args.hreduce);
        if (a == 0 && c < NR && mine) pool[c] = pack(sc, grow);
    }
    __syncthreads();
    // the k-th best exact entry by rank (keys are unique: exactly one entry has each rank)
    if (tid < 256) keys[tid] = pool[tid] != kEmpty ? sortkey(pool[tid]) : 0ull;
    __syncthreads();
    if (tid < NR) {
        const u64 mine = keys[tid];
        if (mine != 0ull) {
            int greater = 0;
#pragma unroll 8
            for (int j = 0; j < NR; ++j) greater += keys[j] > mine ? 1 : 0;
            if (greater == k - 1) s_kth = pool[tid];
        }
    }
    __syncthreads();
    if (tid == 0) {
        float t = -INFINITY;   // fewer than k rows: everything is a candidate (the main pass's lists then overflow into the exact path)
        if (d < 0.f || !real_query) {
            t = INFINITY;      // skipped query (padding / zero / non-finite): the exact path answers it
            if (args.overflow) args.overflow[q] = 1;
        } else {
            // the k-th best group maximum: k distinct rows score at least that (approximately); the sample pass takes its maxima over
            // live, allowed rows only (a group whose rows are all filtered out reports nothing)
            const u64 ak = k <= M ? top[k - 1] : kEmpty;
            if (ak != kEmpty) {
                const float ta = __uint_as_float((uint32_t)(ak >> 32)) - 2.0f * d;
                if (ta == ta) t = ta;
            }
            const u64 kth = s_kth;
            if (kth != 0ull) {
                const float sk = __uint_as_float((uint32_t)(kth >> 32));
                const float v = sk * args.anchor_unit[q];
                const float te = v - d - fabsf(v) * 1e-6f - 1.0f;
                if (te == te && te > t) t = te;
            }
        }
        args.tau_out[q] = t;
        if (args.spill_reset) args.spill_reset[(size_t)q * kMfmaSpillCountStride] = 0u;
    }
}

bool select_groups_args_ok(const GroupSelectArgs& args) {
    if (args.k < 1 || args.nentries == 0 || args.nentries > 1024 || !args.delta || !args.tau_out) return false;
    if (args.rank_only ? args.k > kGroupsRankMax : (args.k > kGroupsTakenMax || (args.dim & 7) || args.dim > kSelQueryLds || !args.anchor_unit || !args.slab))
        return false;
    return true;
}

hipError_t launch_select_groups(const GroupSelectArgs& args, int nq, hipStream_t stream) {
    if (!select_groups_args_ok(args)) return hipErrorInvalidValue;
    constexpr int M0 = (int)kGroupsTaken, M1 = (int)kGroupsTakenMax;
    if (args.rank_only) {
        if (args.k <= 64) hipLaunchKernelGGL((select_groups_kernel<true, M0, 64>), dim3(nq), dim3(512), 0, stream, args);
        else hipLaunchKernelGGL((select_groups_kernel<true, M0, (int)kGroupsRankMax>), dim3(nq), dim3(512), 0, stream, args);
    } else {
        if (args.slab_f32) {
            if (args.k <= kGroupsTaken) hipLaunchKernelGGL((select_groups_kernel<false, M0, 64, true>), dim3(nq), dim3(512), 0, stream, args);
            else hipLaunchKernelGGL((select_groups_kernel<false, M1, 64, true>), dim3(nq), dim3(512), 0, stream, args);
        } else if (args.k <= kGroupsTaken) hipLaunchKernelGGL((select_groups_kernel<false, M0, 64>), dim3(nq), dim3(512), 0, stream, args);
        else hipLaunchKernelGGL((select_groups_kernel<false, M1, 64>), dim3(nq), dim3(512), 0, stream, args);
    }
    return hipGetLastError();
}

__global__ __launch_bounds__(256) void list_cut_kernel(const u64* __restrict__ lists, uint32_t nlists, uint32_t list_len, float* __restrict__ out) {
    __shared__ u64 red[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    u64 m = 0;
    for (uint32_t l = tid; l < nlists; l += 256) {
        const u64 e = lists[(size_t)l * list_len + list_len - 1];
        const u64 key = e != kEmpty ? sortkey(e) : 0ull;
        m = key > m ? key : m;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const u64 o = __shfl_xor(m, off);
        m = o > m ? o : m;
    }
    if (lane == 0) red[wave] = m;
    __syncthreads();
    if (tid == 0) {
#pragma unroll
        for (int w = 1; w < 4; ++w) m = red[w] > m ? red[w] : m;
        out[0] = m ? __uint_as_float(score_from_sortkey(m)) : -INFINITY;
    }
}

bool list_cut_args_ok(uint32_t nlists, uint32_t list_len) {
    (void)nlists;
    return list_len != 0;
}

hipError_t launch_list_cut(const u64* lists, uint32_t nlists, uint32_t list_len, float* out, hipStream_t stream) {
    if (!list_cut_args_ok(nlists, list_len)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(list_cut_kernel, dim3(1), dim3(256), 0, stream, lists, nlists, list_len, out);
    return hipGetLastError();
}

bool select_args_ok(const SelectArgs& args) {
    if (args.k < 1 || args.k > kSelectMaxK || !args.delta || (uint64_t)args.nlists * args.list_len > 0x7fffffffull) return false;
    if (args.slab) {
        if (args.k_out < 1 || args.k_out > 64 || (args.dim & 7)) return false;
        if (args.slab_f32 && args.row_stride && args.row_stride != args.dim * 4) return false;   // dense f32 rows only (no MRL prefix views of F32 slabs here)
    }
    return true;
}

hipError_t launch_select(const SelectArgs& args, int nq, hipStream_t stream) {
    if (!select_args_ok(args)) return hipErrorInvalidValue;
#ifdef FSGPU_EXPERIMENTS
    static const int sort_above = [] {
        const char* e = std::getenv("FSGPU_SELECT_SORT_ABOVE");  // tuning experiments only
        return e ? std::atoi(e) : 32;
    }();
#else
    constexpr int sort_above = 32;   // ranks above it compact + bitonic-sort instead of extracting
#endif
    const bool sorted = (int)args.k > sort_above || args.k > 64 || (args.big_pool && args.slab && !args.take_topk);
    constexpr size_t sort_lds = (size_t)kSelSortCap * 8;
    static bool attr_done = false;
    if (!attr_done) {  // 64 KB of dynamic LDS on top of the static arrays needs the opt-in
        hipError_t e1 = hipFuncSetAttribute(reinterpret_cast<const void*>(select_kernel<true, true>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds);
        hipError_t e2 = hipFuncSetAttribute(reinterpret_cast<const void*>(select_kernel<false, true>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds);
        hipError_t e3 = hipFuncSetAttribute(reinterpret_cast<const void*>(select_kernel<true, true, true>),
                                            hipFuncAttributeMaxDynamicSharedMemorySize, (int)sort_lds);
        if (e1 != hipSuccess) return e1;
        if (e2 != hipSuccess) return e2;
        if (e3 != hipSuccess) return e3;
        attr_done = true;
    }
    if (args.slab) {
        if (args.slab_f32) {
            if (sorted) hipLaunchKernelGGL((select_kernel<true, true, true>), dim3(nq), dim3(kSelThreads), sort_lds, stream, args);
            else hipLaunchKernelGGL((select_kernel<true, false, true>), dim3(nq), dim3(kSelThreads), 0, stream, args);
            return hipGetLastError();
        }
        if (sorted) hipLaunchKernelGGL((select_kernel<true, true>), dim3(nq), dim3(kSelThreads), sort_lds, stream, args);
        else hipLaunchKernelGGL((select_kernel<true, false>), dim3(nq), dim3(kSelThreads), 0, stream, args);
    } else {
        if (sorted) hipLaunchKernelGGL((select_kernel<false, true>), dim3(nq), dim3(kSelThreads), sort_lds, stream, args);
        else hipLaunchKernelGGL((select_kernel<false, false>), dim3(nq), dim3(kSelThreads), 0, stream, args);
    }
    return hipGetLastError();
}

hipError_t launch_max_row_norm(const void* slab, uint32_t nrows, uint32_t dim, uint32_t row_stride_bytes, unsigned int* out_bits,
                               hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out_bits, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(max_row_norm_kernel, dim3(2048), dim3(256), 0, stream, static_cast<const unsigned short*>(slab),
                       nrows, dim, row_stride_bytes ? row_stride_bytes / 2 : dim, out_bits);
    return hipGetLastError();
}

hipError_t launch_max_row_norm_f32(const float* rows, uint32_t nrows, uint32_t dim, unsigned int* out_bits, hipStream_t stream) {
    hipError_t e = hipMemsetAsync(out_bits, 0, 4, stream);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(max_row_norm_f32_kernel, dim3(2048), dim3(256), 0, stream, rows, nrows, dim, out_bits);
    return hipGetLastError();
}

hipError_t launch_prepare_queries(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t q_stride,
                                  const unsigned int* max_norm_bits, void* qh, float* delta, hipStream_t stream) {
    hipLaunchKernelGGL(prepare_queries_kernel, dim3(nq_pad), dim3(256), 0, stream, q, nq, q_stride ? q_stride : dim, dim, max_norm_bits,
                       static_cast<_Float16*>(qh), delta);
    return hipGetLastError();
}

}  // namespace fsgpu

// search_hits_kernels.hip — the WAL half and the resolve step of the batched search_hits (vector_index_hits.cpp):
// scan_wal (crates/frankensearch-index/src/search.rs:1449-1475) and resolve_hits (:1493-1558) for a whole batch of queries.
//
// wal_topk_kernel: dot_product_f32_f32 (simd.rs:134-222) of every resident WAL entry with the block's queries — four 8-lane
// accumulators over groups of 32 elements, separate multiply and add (this file is compiled with -ffp-contract=off like the
// others), (acc0+acc1)+(acc2+acc3), the leftover 8-element chunks into that sum, reduce_add, and for the last dim % 8 elements a
// multiply and an add (NOT the fused multiply-add of the f32 slab's dot_product_f32_bytes_f32: the only place where this kernel's
// arithmetic differs from scan_topk_f32_kernel, f32_kernels.hip) — and each query's kw best finite scores.
// Mapping as in f32_kernels.hip: a quad of lanes per entry, lane a owns accumulator a (the quad reads 128 contiguous bytes), the
// combine is two DPP quad butterflies, leftovers and tail are computed redundantly by the quad; threshold-gated wave candidate
// buffers (one per query) and a block fold.  The WAL is small (at most a few thousand rows, resident in L2), so the kernel is
// latency-bound: the grid is sized by the queries (NQ per block), every block walks the whole WAL.
//
// resolve_hits_kernel: one wave per query merges the query's best-first main list with its WAL list, keeps the first k and applies
// the three drops of resolve_hits in the reference's order; doc ids are their CLASS numbers here (compared as bytes once, on the
// host, when the tables are built).
#include <atomic>

#include "kernels.hpp"
#include "scan_common.hpp"

namespace fsgpu {

using namespace scan_detail;

template <int KCAP, int NQ>
__global__ __launch_bounds__(256) void wal_topk_kernel(WalTopkArgs args) {
    constexpr int CAP = 2 * KCAP;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int dim = (int)args.dim;
    float* qs = reinterpret_cast<float*>(smem);                                                      // [NQ][dim]
    u64* bufs = reinterpret_cast<u64*>(smem + (((size_t)NQ * dim * 4 + 15) & ~(size_t)15));         // [wave][NQ][CAP]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int a = lane & 3, r = lane >> 2;
    const uint32_t q0 = blockIdx.x * NQ;   // (< nq: the grid is ceil(nq / NQ))
    for (int i = tid; i < NQ * dim; i += 256) {
        const uint32_t q = q0 + (uint32_t)(i / dim);
        qs[i] = args.queries[(size_t)(q < args.nq ? q : args.nq - 1) * dim + (i % dim)];   // (a short last block repeats the last query)
    }
    __syncthreads();
    WaveTopK<CAP> tk[NQ];
    u64 thr[NQ];
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        tk[q].init(bufs + ((size_t)wave * NQ + q) * CAP);
        thr[q] = 0;
    }
    const uint32_t W = args.W;
    const uint32_t ntiles = (W + kRowsPerTile - 1) / kRowsPerTile;
    const bool vec = (dim & 3) == 0;   // 16-byte aligned rows: dwordx4 loads
    const int k = (int)args.kw;
    const int chunks = dim >> 3, groups = chunks >> 2;
    for (uint32_t tile = wave; tile < ntiles; tile += kWavesPerBlock) {
        const uint32_t row = tile * kRowsPerTile + r;
        const uint32_t rowc = row < W ? row : W - 1;
        const float* w = args.wal + (size_t)rowc * dim;
        float acc[NQ][8];
#pragma unroll
        for (int q = 0; q < NQ; ++q)
#pragma unroll
            for (int j = 0; j < 8; ++j) acc[q][j] = 0.f;
#pragma unroll 2
        for (int g = 0; g < groups; ++g) {
            const int e = 32 * g + 8 * a;
            float x[8];
            if (vec) {
                const float4 lo = *reinterpret_cast<const float4*>(w + e), hi = *reinterpret_cast<const float4*>(w + e + 4);
                x[0] = lo.x; x[1] = lo.y; x[2] = lo.z; x[3] = lo.w;
                x[4] = hi.x; x[5] = hi.y; x[6] = hi.z; x[7] = hi.w;
            } else {
#pragma unroll
                for (int j = 0; j < 8; ++j) x[j] = w[e + j];
            }
#pragma unroll
            for (int q = 0; q < NQ; ++q)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = x[j] * qs[q * dim + e + j];
                    acc[q][j] = acc[q][j] + p;
                }
        }
#pragma unroll
        for (int q = 0; q < NQ; ++q) {
            float v[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float u = acc[q][j] + quad_xor1(acc[q][j]);
                v[j] = u + quad_xor2(u);
            }
            for (int c = 4 * groups; c < chunks; ++c)   // leftover chunks join AFTER the combine (simd.rs:134-222)
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const float p = w[8 * c + j] * qs[q * dim + 8 * c + j];
                    v[j] = v[j] + p;
                }
            float score = hreduce8(v, args.hreduce);
            for (int i = chunks * 8; i < dim; ++i) {    // the scalar tail: a multiply, then an add
                const float p = w[i] * qs[q * dim + i];
                score = score + p;
            }
            const bool mine = a == 0 && row < W && q0 + (uint32_t)q < args.nq;
            if (args.out_scores && mine) args.out_scores[(size_t)(q0 + q) * W + row] = score;
            if (!args.out_packed) continue;   // (uniform)
            const bool finite = (__float_as_uint(score) & 0x7f800000u) != 0x7f800000u;   // search.rs:1466-1470, before packing
            const u64 packed = pack(score, args.nrows + row);
            bool cand = mine && finite && sortkey(packed) > thr[q];
            u64 m = __ballot(cand);
            if (m == 0) continue;
            if (tk[q].count + (int)__popcll(m) > CAP) {
                thr[q] = tk[q].compact(k, lane);
                cand = cand && sortkey(packed) > thr[q];
                m = __ballot(cand);
            }
            if (cand) tk[q].buf[tk[q].count + (int)__popcll(m & ((1ull << lane) - 1ull))] = packed;
            tk[q].count += (int)__popcll(m);
        }
    }
    if (!args.out_packed) return;   // (uniform)
#pragma unroll
    for (int q = 0; q < NQ; ++q) (void)tk[q].compact(k, lane);
    __syncthreads();
    // fold the four waves' best-first lists of a query: elementwise max of A[i] and B[KCAP-1-i], re-sort.  Wave q folds query q
    // (NQ <= 4 = the block's waves); its destination is wave 0's buffer of that query.
    if (wave < NQ && q0 + (uint32_t)wave < args.nq) {
        const int q = wave;
        u64* dst = bufs + (size_t)q * CAP;
        for (int w = 1; w < kWavesPerBlock; ++w) {
            const u64* src = bufs + ((size_t)w * NQ + q) * CAP;
            for (int i = lane; i < KCAP; i += 64) {
                const u64 xx = dst[i], yy = src[KCAP - 1 - i];
                dst[i] = sortkey(xx) >= sortkey(yy) ? xx : yy;
            }
            for (int i = KCAP + lane; i < CAP; i += 64) dst[i] = kEmpty;
            wave_sort_desc<CAP>(dst, lane);
        }
        u64* out = args.out_packed + (size_t)(q0 + q) * k;
        for (int i = lane; i < k; i += 64) out[i] = dst[i];
    }
}

constexpr size_t kWalLdsMax = (size_t)144 * 1024;   // of the CU's 160 KB, as the F32 scan (f32_kernels.hip)

static size_t wal_topk_lds(int dim, int kcap, int nq) {
    return (((size_t)nq * dim * 4 + 15) & ~(size_t)15) + (size_t)kWavesPerBlock * nq * 2 * kcap * 8;
}

template <int KCAP, int NQ>
static hipError_t launch_wal_t(const WalTopkArgs& args, hipStream_t stream) {
    static_assert(NQ <= kWavesPerBlock, "one wave folds one query's lists");
    const size_t lds = wal_topk_lds((int)args.dim, KCAP, NQ);
    auto kern = wal_topk_kernel<KCAP, NQ>;
    // beyond 64 KB the instantiation's limit is raised — once, to the most any supported shape asks for (kWalLdsMax), per device
    static std::atomic<uint64_t> raised{0};
    int dev = 0;
    if (lds > 64 * 1024 && hipGetDevice(&dev) == hipSuccess && dev < 64 && !((raised.load() >> dev) & 1ull)) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kWalLdsMax);
        if (e != hipSuccess) return e;
        raised.fetch_or(1ull << dev);
    }
    hipLaunchKernelGGL(kern, dim3((args.nq + NQ - 1) / NQ), dim3(256), lds, stream, args);
    return hipGetLastError();
}

bool wal_topk_supported(uint32_t dim, uint32_t kw) {
    return dim != 0 && kw != 0 && kw <= kHitsMaxK && wal_topk_lds((int)dim, kw <= 64 ? 64 : 256, 1) <= kWalLdsMax;
}

hipError_t launch_wal_topk(const WalTopkArgs& args, hipStream_t stream) {
    if (args.nq == 0 || args.W == 0 || args.kw > args.W || !wal_topk_supported(args.dim, args.kw)) return hipErrorInvalidValue;
    const int kcap = args.kw <= 64 ? 64 : 256;
    // four queries per block where they and their candidate buffers fit the LDS (the WAL rows are then loaded once for four dots);
    // else one.  A lone score table (lab) keeps no candidates but runs the same code.
    int nq = 0;
    for (int cand : {4, 1})
        if (args.nq >= (uint32_t)cand && wal_topk_lds((int)args.dim, kcap, cand) <= kWalLdsMax) {
            nq = cand;
            break;
        }
    if (nq == 0) nq = 1;   // (fewer than four queries: wal_topk_supported vouched for one per block)
    if (kcap == 64) return nq == 4 ? launch_wal_t<64, 4>(args, stream) : launch_wal_t<64, 1>(args, stream);
    return nq == 4 ? launch_wal_t<256, 4>(args, stream) : launch_wal_t<256, 1>(args, stream);
}

// One wave (= one block) per query.  list[0 .. n): the query's main hits and WAL entries as packed words, n = the power of two
// >= k + kw, sorted best first (a WAL entry's row is nrows + its index: behind every main row of equal score).  Of the first k:
//   1. a main row that is tombstoned is dropped                        (search.rs:1519-1523)
//   2. a main row whose doc id has a resident WAL entry is dropped      (:1524-1531; whether or not that entry made the list)
//   3. a hit whose doc id was emitted before is dropped                 (:1545-1549)
// and nothing refills the list.  Rule 3 over classes: an entry that passed 1 and 2 is emitted iff no EARLIER entry that passed them
// has its class (the first such entry of a class is the emitted one), a prefix compare in LDS.
__global__ __launch_bounds__(64) void resolve_hits_kernel(ResolveHitsArgs args) {
    __shared__ u64 list[2 * kHitsMaxK];
    __shared__ uint32_t cls[kHitsMaxK];
    constexpr uint32_t kNoClass = 0xffffffffu;   // (classes are < nrows + W < 2^32 - 1)
    const int lane = threadIdx.x;
    const uint32_t q = blockIdx.x;
    const int k = (int)args.k, kw = (int)args.kw;
    int n = 2;
    while (n < k + kw) n <<= 1;
    const uint32_t mc = min(args.main_counts[q], args.k);
    for (int i = lane; i < n; i += 64) {
        u64 e = kEmpty;
        if (i < k) {
            if ((uint32_t)i < mc) e = pack(args.main_scores[(size_t)q * k + i], args.main_rows[(size_t)q * k + i]);
        } else if (i < k + kw) {
            e = args.wal_packed[(size_t)q * kw + (i - k)];
        }
        list[i] = e;
    }
    wave_sort_desc_rt(list, n, lane);   // (a merge of two sorted lists would do; at most 512 entries either way)
    for (int i = lane; i < k; i += 64) {
        const u64 e = list[i];
        uint32_t c = kNoClass;
        if (e != kEmpty) {
            const uint32_t row = (uint32_t)e;
            if (row >= args.nrows) {
                c = args.wal_class[row - args.nrows];
            } else {
                bool keep = true;
                if (args.live) keep = (args.live[row >> 6] >> (row & 63)) & 1ull;
                if (keep && args.shadowed) keep = !((args.shadowed[row >> 6] >> (row & 63)) & 1ull);
                if (keep) c = args.main_class[row];
            }
        }
        cls[i] = c;
    }
    wave_lds_fence();
    uint32_t base = 0;
    for (int i0 = 0; i0 < k; i0 += 64) {   // (uniform trip count: the ballot below is taken by the whole wave)
        const int i = i0 + lane;
        bool emit = false;
        u64 e = kEmpty;
        if (i < k) {
            const uint32_t c = cls[i];
            emit = c != kNoClass;
            for (int j = 0; emit && j < i; ++j) emit = cls[j] != c;
            e = list[i];
        }
        const u64 m = __ballot(emit);
        if (emit) {
            const uint32_t pos = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            args.out_rows[(size_t)q * k + pos] = (uint32_t)e;
            args.out_scores[(size_t)q * k + pos] = __uint_as_float((uint32_t)(e >> 32));
        }
        base += (uint32_t)__popcll(m);
    }
    for (int i = (int)base + lane; i < k; i += 64) {
        args.out_rows[(size_t)q * k + i] = 0;
        args.out_scores[(size_t)q * k + i] = 0.f;
    }
    if (lane == 0) args.out_counts[q] = base;
}

hipError_t launch_resolve_hits(const ResolveHitsArgs& args, hipStream_t stream) {
    if (args.nq == 0 || args.k == 0 || args.k > kHitsMaxK || args.kw > kHitsMaxK) return hipErrorInvalidValue;
    hipLaunchKernelGGL(resolve_hits_kernel, dim3(args.nq), dim3(64), 0, stream, args);
    return hipGetLastError();
}

}  // namespace fsgpu

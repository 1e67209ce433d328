// ann_kernels.hip — beam search over the exact k-NN table (include/fsgpu.h, "graph ANN search"; ann_index.cpp).
//
// The answer is a pure function of (slab, live bitmap, table, query, parameters); this file computes it with one workgroup of 256
// threads per query and no communication between workgroups.
//   state in LDS   the query as f32; the beam (two buffers of 256 packed entries, swapped by every merge) with the expanded flags
//                  BESIDE the entries; the step's walked ids, admitted rows and admitted entries; the visited set — an
//                  open-addressing table of local rows, inserted with a compare-and-swap: the lane that inserts a row owns it.
//                  Entry rows do not occupy the table: membership in the strided entry set is arithmetic (is_entry_row).
//   a step         select (ballot + wave counts: the first `expand` unexpanded entries in beam order) -> walk (one thread per
//                  (list, column); the first pad of a list by an LDS atomicMin) -> admit (bounds, live bit, entry set, table) ->
//                  score (a quad of lanes per row, 64 rows per pass, the arithmetic of gather_dot_kernel / dot_rows_f32_kernel)
//                  -> sort the admitted entries (block_sort_desc_rt) -> merge by rank: an entry's place is its index in its own
//                  sorted list plus the number of entries of the other list that beat it; keys are distinct, so the places are too.
// Which lane wins an insertion and where an admitted row lands before the sort vary from run to run; the sorted list, and so the
// beam, do not.  Every table, list and row index is checked against nrows before it is used as an address.
#include "kernels.hpp"
#include "scan_common.hpp"

namespace fsgpu {

using namespace scan_detail;

namespace {

constexpr int kAnnThreads = 256;
constexpr uint32_t kAnnFree = 0xffffffffu;   // a free slot of the visited table (no row has this id)
constexpr int kAnnBatchF16 = 12;             // groups of 32 elements whose loads are in flight per lane: all of a 384-dimension row
constexpr int kAnnBatchF32 = 6;

// LDS layout behind the query (all offsets multiples of 16)
constexpr size_t kOffBeam = 0;                                            // [2][256] u64
constexpr size_t kOffCand = kOffBeam + 2 * kAnnMaxEf * 8;                 // [512] u64 admitted entries
constexpr size_t kOffTable = kOffCand + kAnnMaxStepRows * 8;              // [8192] u32
constexpr size_t kOffWalk = kOffTable + kAnnTableSlots * 4;               // [512] u32 walked ids (global)
constexpr size_t kOffAdmit = kOffWalk + kAnnMaxStepRows * 4;              // [512] u32 admitted rows (local)
constexpr size_t kOffFlags = kOffAdmit + kAnnMaxStepRows * 4;             // [2][256] u8
constexpr size_t kOffSmall = kOffFlags + 2 * kAnnMaxEf;                   // sel[8] | stop[8] | wave counts[4] | admitted count | pad
constexpr size_t kAnnStateBytes = kOffSmall + 24 * 4;

// r = floor(i * n / n_entry) for some i < n_entry?  (n_entry <= n: the entry rows are distinct and i is unique)
__device__ __forceinline__ bool is_entry_row(uint32_t r, uint32_t n, uint32_t n_entry) {
    const u64 i = ((u64)r * n_entry + n - 1) / n;
    return i < n_entry && (uint32_t)(i * n / n_entry) == r;
}

// dot_product_f16_bytes_f32 of one row on a quad of lanes, in gather_dot_kernel's operation order (scan_kernels.hip): lane a owns
// accumulator a, the leftover chunks go to accumulator 0 before the combine, a fused multiply-add per element of the last dim % 8.
// vec: 16-byte aligned rows of whole chunks (dwordx4 loads); else element loads — the same arithmetic either way.
template <int BATCH>
__device__ __forceinline__ float quad_dot_f16(const unsigned char* rowp, const float* qs, int dim, int a, bool vec, int hreduce) {
    const int chunks = dim >> 3, groups = chunks >> 2;
    float acc[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) acc[j] = 0.f;
    if (vec) {
        const u32x4* p = reinterpret_cast<const u32x4*>(rowp);
        for (int g0 = 0; g0 < groups; g0 += BATCH) {
            u32x4 w[BATCH];
#pragma unroll
            for (int b = 0; b < BATCH; ++b)
                if (g0 + b < groups) w[b] = p[4 * (g0 + b) + a];
#pragma unroll
            for (int b = 0; b < BATCH; ++b)
                if (g0 + b < groups) {
                    const float4* qp = reinterpret_cast<const float4*>(qs + 32 * (g0 + b) + 8 * a);
                    chunk_mac(acc, w[b], qp[0], qp[1]);
                }
        }
        if (a == 0)
            for (int c = 4 * groups; c < chunks; ++c) {
                const u32x4 w = p[c];
                const float4* qp = reinterpret_cast<const float4*>(qs + 8 * c);
                chunk_mac(acc, w, qp[0], qp[1]);
            }
        return quad_finish(acc, hreduce);   // (dim % 8 == 0 here: no tail)
    }
    const _Float16* hp = reinterpret_cast<const _Float16*>(rowp);
    for (int g = 0; g < groups; ++g)
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int e = 32 * g + 8 * a + j;
            const float p = (float)hp[e] * qs[e];
            acc[j] = acc[j] + p;
        }
    if (a == 0)
        for (int c = 4 * groups; c < chunks; ++c)
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const float p = (float)hp[8 * c + j] * qs[8 * c + j];
                acc[j] = acc[j] + p;
            }
    float s = quad_finish(acc, hreduce);
    for (int i = chunks * 8; i < dim; ++i) s = __builtin_fmaf((float)hp[i], qs[i], s);
    return s;
}

// entries of the sorted list `other` (n real entries, best first) that beat `key`
__device__ __forceinline__ uint32_t count_better(const u64* other, uint32_t n, u64 key) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sortkey(other[mid]) > key) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

template <bool F32>
__global__ __launch_bounds__(kAnnThreads) void ann_search_kernel(AnnSearchArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, quad = tid >> 2;
    const int qa = (int)(tid & 3u);
    const uint32_t q = blockIdx.x;
    const uint32_t n = a.nrows, dim = a.dim, ef = a.ef, degree = a.degree;
    float* qs = reinterpret_cast<float*>(smem);
    unsigned char* st = smem + (((size_t)dim * 4 + 15) & ~(size_t)15);
    u64* cur = reinterpret_cast<u64*>(st + kOffBeam);
    u64* nxt = cur + kAnnMaxEf;
    u64* cand = reinterpret_cast<u64*>(st + kOffCand);
    uint32_t* table = reinterpret_cast<uint32_t*>(st + kOffTable);
    uint32_t* walk = reinterpret_cast<uint32_t*>(st + kOffWalk);
    uint32_t* admit = reinterpret_cast<uint32_t*>(st + kOffAdmit);
    unsigned char* cur_flag = st + kOffFlags;
    unsigned char* nxt_flag = cur_flag + kAnnMaxEf;
    uint32_t* sel = reinterpret_cast<uint32_t*>(st + kOffSmall);
    uint32_t* stop = sel + 8;
    uint32_t* wave_count = stop + 8;
    uint32_t* n_admit_s = wave_count + 4;

    for (uint32_t i = tid; i < dim; i += kAnnThreads) qs[i] = a.queries[(size_t)q * dim + i];
    for (uint32_t i = tid; i < kAnnTableSlots; i += kAnnThreads) table[i] = kAnnFree;
    if (tid == 0) *n_admit_s = 0;
    __syncthreads();

    const unsigned char* slab = static_cast<const unsigned char*>(a.slab);
    const bool vec = (a.row_stride & 15u) == 0 && (reinterpret_cast<uintptr_t>(a.slab) & 15u) == 0 && (F32 || (dim & 7u) == 0);
    uint32_t n_beam = 0, scored = 0, steps = 0;   // block-uniform

    // admit[0 .. n_admit) hold distinct local rows that are not in the beam: score them, sort them, merge them into the beam
    auto score_and_merge = [&](uint32_t n_admit) {
        for (uint32_t base = 0; base < n_admit; base += kAnnThreads / 4) {
            const uint32_t item = base + quad;
            if (item < n_admit) {   // (a quad is in or out as a whole)
                uint32_t row = admit[item];
                if (row >= n) row = 0;   // cannot happen: admitted rows were checked
                const unsigned char* rowp = slab + (size_t)row * a.row_stride;
                float s;
                if constexpr (F32)
                    s = quad_dot_f32<kAnnBatchF32>(reinterpret_cast<const float*>(rowp), qs, (int)dim, qa, vec, a.hreduce);
                else
                    s = quad_dot_f16<kAnnBatchF16>(rowp, qs, (int)dim, qa, vec, a.hreduce);
                if (qa == 0) cand[item] = pack(s, a.row_base + row);
            }
        }
        uint32_t npow = 2;
        while (npow < n_admit) npow <<= 1;
        for (uint32_t i = n_admit + tid; i < npow; i += kAnnThreads) cand[i] = kEmpty;
        block_sort_desc_rt<kAnnThreads>(cand, (int)npow, (int)tid);   // (barrier first, barrier last)
        if (tid < n_beam) {
            const u64 e = cur[tid];
            const uint32_t pos = tid + count_better(cand, n_admit, sortkey(e));
            if (pos < ef) {
                nxt[pos] = e;
                nxt_flag[pos] = cur_flag[tid];
            }
        }
        for (uint32_t c = tid; c < n_admit; c += kAnnThreads) {
            const u64 e = cand[c];
            const uint32_t pos = c + count_better(cur, n_beam, sortkey(e));
            if (pos < ef) {
                nxt[pos] = e;
                nxt_flag[pos] = 0;
            }
        }
        n_beam = n_beam + n_admit < ef ? n_beam + n_admit : ef;
        u64* t = cur; cur = nxt; nxt = t;
        unsigned char* tf = cur_flag; cur_flag = nxt_flag; nxt_flag = tf;
        __syncthreads();
    };

    // ---- entry: the live rows floor(i * n / n_entry), in blocks of kAnnMaxStepRows ----
    for (uint32_t base = 0; base < a.n_entry; base += kAnnMaxStepRows) {
        for (uint32_t c = tid; c < kAnnMaxStepRows && base + c < a.n_entry; c += kAnnThreads) {
            const uint32_t e = (uint32_t)((u64)(base + c) * n / a.n_entry);
            if (e < n && row_live(a.live, e)) admit[atomicAdd(n_admit_s, 1u)] = e;
        }
        __syncthreads();
        const uint32_t n_admit = *n_admit_s;
        __syncthreads();
        if (tid == 0) *n_admit_s = 0;
        scored += n_admit;
        if (n_admit) score_and_merge(n_admit);
        else __syncthreads();
    }

    // ---- steps ----
    for (uint32_t it = 0; it < a.max_iters; ++it) {
        // select: the first `expand` unexpanded entries in beam order
        const bool unexpanded = tid < n_beam && !cur_flag[tid];
        const unsigned long long ballot = __ballot(unexpanded);
        if (lane == 0) wave_count[wave] = (uint32_t)__popcll(ballot);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kAnnThreads / 64; ++w) {
            const uint32_t c = wave_count[w];
            if (w < wave) before += c;
            total += c;
        }
        if (total == 0) break;   // block-uniform
        const uint32_t n_sel = total < a.expand ? total : a.expand;
        const uint32_t rank = before + (uint32_t)__popcll(ballot & ((1ull << lane) - 1ull));
        if (unexpanded && rank < n_sel) {
            sel[rank] = (uint32_t)cur[tid] - a.row_base;
            cur_flag[tid] = 1;
        }
        if (tid < kAnnMaxExpand) stop[tid] = degree;
        __syncthreads();
        // walk: thread c reads column c % degree of list c / degree; the first pad of a list ends it
        const uint32_t n_walk = n_sel * degree;   // <= kAnnMaxStepRows
        for (uint32_t c = tid; c < n_walk; c += kAnnThreads) {
            const uint32_t l = c / degree, col = c - l * degree;
            const uint32_t parent = sel[l];
            const uint32_t id = parent < n ? a.graph[(size_t)parent * a.width + col] : kKnnPadRow;
            walk[c] = id;
            if (id == kKnnPadRow) atomicMin(&stop[l], col);
        }
        __syncthreads();
        // admit: inside the index, live, not an entry row (the live ones are visited), not in the table yet
        for (uint32_t c = tid; c < n_walk; c += kAnnThreads) {
            const uint32_t l = c / degree, col = c - l * degree;
            if (col >= stop[l]) continue;
            const uint32_t row = walk[c] - a.row_base;   // wraps for ids below the base
            if (row >= n || !row_live(a.live, row) || is_entry_row(row, n, a.n_entry)) continue;
            uint32_t h = (row * 2654435761u) >> 19;   // 13 bits: kAnnTableSlots
            bool mine = false;
            for (uint32_t probe = 0; probe < kAnnTableSlots; ++probe) {
                const uint32_t old = atomicCAS(&table[h], kAnnFree, row);
                if (old == kAnnFree) {
                    mine = true;
                    break;
                }
                if (old == row) break;   // visited in an earlier step, or reached twice in this one
                h = (h + 1u) & (kAnnTableSlots - 1u);
            }
            if (mine) {
                const uint32_t slot = atomicAdd(n_admit_s, 1u);
                if (slot < kAnnMaxStepRows) admit[slot] = row;
            }
        }
        __syncthreads();
        uint32_t n_admit = *n_admit_s;
        if (n_admit > kAnnMaxStepRows) n_admit = kAnnMaxStepRows;   // cannot happen: n_walk <= kAnnMaxStepRows
        __syncthreads();
        if (tid == 0) *n_admit_s = 0;
        steps += 1;
        scored += n_admit;
        if (n_admit) score_and_merge(n_admit);
        else __syncthreads();
    }

    const uint32_t count = n_beam < a.k ? n_beam : a.k;
    for (uint32_t i = tid; i < a.k; i += kAnnThreads) {
        const u64 e = i < count ? cur[i] : kEmpty;
        a.out_rows[(size_t)q * a.k + i] = i < count ? (uint32_t)e : kKnnPadRow;
        a.out_scores[(size_t)q * a.k + i] = i < count ? __uint_as_float((uint32_t)(e >> 32)) : 0.0f;
    }
    if (tid == 0) {
        a.out_counts[q] = count;
        a.out_scored[q] = scored;
        a.out_steps[q] = steps;
    }
}

static_assert(kAnnTableSlots == 1u << 13, "the hash keeps 13 bits");
static_assert(kAnnMaxAdmitted * 2 <= kAnnTableSlots, "the visited table stays at most half full");
static_assert(kAnnMaxEf == kAnnThreads, "one thread per beam entry in the select and merge steps");

}  // namespace

size_t ann_lds_bytes(uint32_t dim) { return (((size_t)dim * 4 + 15) & ~(size_t)15) + kAnnStateBytes; }

bool ann_args_ok(const AnnSearchArgs& a) {
    if (!a.slab || !a.graph || !a.queries || !a.out_rows || !a.out_scores || !a.out_counts || !a.out_scored || !a.out_steps) return false;
    if (a.nrows == 0 || a.dim == 0 || a.dim > kAnnMaxDim) return false;
    if (a.k < 1 || a.k > a.ef || a.ef > kAnnMaxEf) return false;
    if (a.expand < 1 || a.expand > kAnnMaxExpand || a.max_iters < 1) return false;
    if (a.degree < 1 || a.degree > a.width) return false;
    if ((uint64_t)a.expand * a.degree > kAnnMaxStepRows) return false;
    if ((uint64_t)a.max_iters * a.expand * a.degree > kAnnMaxAdmitted) return false;
    if (a.n_entry < 1 || a.n_entry > a.nrows || a.n_entry > kAnnMaxEntry) return false;
    if (a.row_stride < a.dim * (a.slab_f32 ? 4u : 2u)) return false;
    return true;
}

template <bool F32>
static hipError_t ann_prepare(size_t lds) {
    if (lds > 64 * 1024)
        return hipFuncSetAttribute(reinterpret_cast<const void*>(ann_search_kernel<F32>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    return hipSuccess;
}

hipError_t launch_ann_search(const AnnSearchArgs& a, uint32_t nq, hipStream_t stream) {
    if (nq == 0) return hipSuccess;
    if (!ann_args_ok(a)) return hipErrorInvalidValue;
    const size_t lds = ann_lds_bytes(a.dim);
    const hipError_t e = a.slab_f32 ? ann_prepare<true>(lds) : ann_prepare<false>(lds);
    if (e != hipSuccess) return e;
    if (a.slab_f32) hipLaunchKernelGGL(ann_search_kernel<true>, dim3(nq), dim3(kAnnThreads), lds, stream, a);
    else hipLaunchKernelGGL(ann_search_kernel<false>, dim3(nq), dim3(kAnnThreads), lds, stream, a);
    return hipGetLastError();
}

}  // namespace fsgpu

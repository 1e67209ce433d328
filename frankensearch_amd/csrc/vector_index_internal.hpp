// vector_index_internal.hpp — what the translation units of VectorIndex share: status helpers, the HIP / status early-return
// macros, the switches read from the environment and the batched search's request, outcome, plan, round and ticket.  Not installed,
// not part of the C ABI (include/fsgpu.h is).
//   vector_index.cpp          lifecycle, FSVI image, WAL, tombstones, the exact scan paths, MRL views, packed lists
//   vector_index_batched.cpp  the batched (matrix-core) search: plan, sample, main pass, selections, fallback, tickets, and the
//                             int8 filter's copy of the slab
//   vector_index_compact.cpp  append_batch, compact, vacuum: the plan, the device rewrite of the slab, the tables, the FSVI image
//   vector_index_lone.cpp     one query at a time: the certified int8 pass, the exact halves, the quantised two-pass lanes
//   vector_index_hits.cpp     search_hits for a batch: the doc-id class tables, the WAL mirror, the WAL and resolve kernels' launches
//   vector_index_filtered.cpp a filter per query in one batched call: the plan, the row lists, the segmented gather scan's launch
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>

#include "../../include/fsgpu.h"
#include "vector_index.hpp"

namespace fsgpu {
namespace detail {

inline SearchError ok() { return SearchError{}; }

inline SearchError hip_fail(hipError_t e, const char* what) {
    SearchError err;
    err.code = FSGPU_ERR_DEVICE;
    err.detail = std::string(what) + ": " + hipGetErrorString(e);
    return err;
}

inline SearchError make_error(int32_t code, std::string detail) {
    SearchError e;
    e.code = code;
    e.detail = std::move(detail);
    return e;
}

// CRC-32 (IEEE) of the FSVI header and FNV-1a 64 of a doc id (lib.rs fnv1a_hash): shared by the reader, the writer and rewrite_index
inline uint32_t crc32_ieee(const uint8_t* p, size_t n) {
    static uint32_t table[256];
    static bool init = false;
    if (!init) {
        for (uint32_t i = 0; i < 256; ++i) {
            uint32_t c = i;
            for (int b = 0; b < 8; ++b) c = (c & 1u) ? (0xedb88320u ^ (c >> 1)) : (c >> 1);
            table[i] = c;
        }
        init = true;
    }
    uint32_t c = 0xffffffffu;
    for (size_t i = 0; i < n; ++i) c = table[(c ^ p[i]) & 0xffu] ^ (c >> 8);
    return ~c;
}

inline uint64_t fnv1a(const char* p, size_t n) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i) {
        h ^= (uint8_t)p[i];
        h *= 0x100000001b3ull;
    }
    return h;
}

// Switches read from the environment ONCE (getenv is not safe against concurrent setenv).  A default build reads six:
// FSGPU_WIDE, FSGPU_WIDE_LAYOUT, FSGPU_WIDE_PRIO, FSGPU_WIDE_SYNC, FSGPU_FILTER, FSGPU_DEBUG_BATCHED (documented in include/fsgpu.h).  Everything else is a tuning / A-B knob of the
// lab and exists only in builds with -DFSGPU_EXPERIMENTS (FSGPU_BUILD_DEFS, frankensearch_amd/build.py; scripts/exp_*).
struct Knobs {
    int grid_blocks = 0, ra = 0, rb = 0, mfma_shape = 0, mfma_shape_i8 = 0, round = 0, i8_per_cu = 0;
    int wide = -1;  // FSGPU_WIDE: 0 = never the register-resident-query main pass, 2 / 3 = its query tiles per wave
    bool wide_sequential = false;   // FSGPU_WIDE_LAYOUT=sequential: the query groups of a wide main-pass launch one after the other on the
                                    // whole grid (the layout before the side-by-side one; both can be timed from one build)
    bool wide_flat_priority = false;   // FSGPU_WIDE_PRIO=off: the wide kernels' split loop without its progress-ordered wave priority
                                       // (mfma_wide.hip, kOptFlat: the loop as it was before; both can be timed from one build)
    bool wide_barrier_sync = false;    // FSGPU_WIDE_SYNC=barrier: the wide main pass on 128-row tiles with its block barrier per tile instead of the
                                       // per-slot counters (mfma_wide.hip, kOptBarrier: the loop as it was before; both can be timed from one build)
    int filter = 0;     // FSGPU_FILTER: "f16" (1) / "i8" (2) pin the filter of the exact batched search; unset = automatic
    int slots_b = 0, slots_main = 0;   // FSGPU_SLOTS_B / FSGPU_SLOTS_MAIN: list slots per (query, block) of the wide kernel's stages
    int wide_max = 0;   // FSGPU_WIDE_MAX: cap on the query tiles per wave of the wide main pass (default: what the registers hold)
    int i8f_growth = 0; // FSGPU_I8F_GROWTH: sample growth factor of the int8 filter (default 4)
    bool no_skip_b = false, use_160 = false, debug_batched = false, no_reverse = false, no_wide_b = false, no_anchor = false;
    bool no_big_pool = false, no_heur_b = false, no_group_sample = false;
    bool narrow_i8f = false;   // FSGPU_NARROW_I8F: batches of up to 64 queries of the int8-filtered exact search on the 64-query shape (rounds 2-5)
    int rb_pct = 0;      // FSGPU_RB_PCT: the second sample's size in percent of what the plan chose (tuning experiments only)
    int heur_rank = 0;   // FSGPU_HEUR_RANK: rank of the first sample whose score gates the anchoring-only second sample (default 4)
    int wide_min = 0;    // FSGPU_WIDE_MIN: fewest queries left that take the register-resident-query main pass (default 129)
    Knobs() {
        auto env = [](const char* name) { return std::getenv(name); };
        if (const char* w = env("FSGPU_WIDE")) wide = std::atoi(w);
        if (const char* l = env("FSGPU_WIDE_LAYOUT")) wide_sequential = std::strcmp(l, "sequential") == 0;
        if (const char* o = env("FSGPU_WIDE_PRIO")) wide_flat_priority = std::strcmp(o, "off") == 0;
        if (const char* y = env("FSGPU_WIDE_SYNC")) wide_barrier_sync = std::strcmp(y, "barrier") == 0;
        if (const char* f = env("FSGPU_FILTER")) filter = std::strcmp(f, "f16") == 0 ? 1 : std::strcmp(f, "i8") == 0 ? 2 : 0;
        debug_batched = env("FSGPU_DEBUG_BATCHED") != nullptr;
#ifdef FSGPU_EXPERIMENTS
        auto num = [&](const char* name) {
            const char* e = env(name);
            return e ? std::atoi(e) : 0;
        };
        grid_blocks = num("FSGPU_GRID_BLOCKS");
        ra = num("FSGPU_RA");
        rb = num("FSGPU_RB");
        rb_pct = num("FSGPU_RB_PCT");
        round = num("FSGPU_ROUND");
        i8_per_cu = num("FSGPU_I8_PER_CU");
        mfma_shape = num("FSGPU_MFMA_SHAPE");
        mfma_shape_i8 = num("FSGPU_MFMA_SHAPE_I8");
        i8f_growth = num("FSGPU_I8F_GROWTH");
        wide_max = num("FSGPU_WIDE_MAX");
        wide_min = num("FSGPU_WIDE_MIN");
        slots_b = std::min(num("FSGPU_SLOTS_B"), (int)kWideSlots);
        slots_main = std::min(num("FSGPU_SLOTS_MAIN"), (int)kWideSlots);
        no_skip_b = env("FSGPU_NO_SKIP_B") != nullptr;
        no_wide_b = env("FSGPU_NO_WIDE_B") != nullptr;
        no_anchor = env("FSGPU_NO_ANCHOR") != nullptr;
        no_big_pool = env("FSGPU_NO_BIG_POOL") != nullptr;
        no_heur_b = env("FSGPU_NO_HEUR_B") != nullptr;
        no_group_sample = env("FSGPU_NO_GROUP_SAMPLE") != nullptr;
        narrow_i8f = env("FSGPU_NARROW_I8F") != nullptr;
        heur_rank = num("FSGPU_HEUR_RANK");
        no_reverse = env("FSGPU_NO_REVERSE") != nullptr;
        use_160 = env("FSGPU_USE_160") != nullptr;
#endif
    }
};
inline const Knobs& knobs() {
    static const Knobs k;
    return k;
}
// Fewest queries that ride the register-resident-query main pass: one more than the LDS-query kernel answers in ONE pass over the slab
// (the tail of a 256-slot launch is padding — batched_round_setup).
// The int8 TWO-PASS (its own pass-1 scores, no anchored threshold) crosses over earlier: 65..128 queries cost 0.86-0.89 ms on the 128-slot
// LDS-query shape and 0.82 ms as a padded 256-slot pass at 10M x 256 (profiles/r06/lds_query_shape_ab.txt).
inline uint32_t wide_min_queries(bool two_pass = false) {
    if (knobs().wide_min > 64) return (uint32_t)knobs().wide_min;
    return two_pass ? 65u : 129u;
}

}  // namespace detail

// ---- the batched (matrix-core) search: what a call asks for, reports and fixes for its rounds; a begun search -------------------
// int8_mult == 0: f16 slab, f16-rounded queries, approximate scores + proven margin (mfma_scan.hip header).
// int8_mult >= 1: int8 slab, int8 queries, exact integer scores; the k * int8_mult best rows are the candidates.
// i8_filter (int8_mult == 0): int8 slab and queries as the FILTER of the exact search — integer scores + the proven margin of
//                 prepare_queries_i8_filter_kernel; queries it cannot certify are re-filtered on the f16 path (refiltered) — on an
//                 F32 slab, whose candidates are re-scored from f32 rows and which has no f16 path, answered by the exact f32 kernels.
struct VectorIndex::BatchedRequest {
    BatchedRequest() = default;   // (a plan's before batched_impl fills it in)
    // what every search names, in the order the entry points of VectorIndex take it; everything else is set by name
    BatchedRequest(const float* queries, uint32_t nq_, uint32_t query_len_, uint32_t k_, hipStream_t stream_)
        : queries_dev(queries), nq(nq_), query_len(query_len_), k(k_), stream(stream_) {}
    const float* queries_dev = nullptr;
    uint32_t nq = 0, query_len = 0, k = 0;
    hipStream_t stream = nullptr;
    const uint64_t* allow_dev = nullptr;
    uint32_t *out_rows_dev = nullptr, *out_counts_dev = nullptr;
    float* out_scores_dev = nullptr;
    uint64_t* out_packed_dev = nullptr;
    uint32_t int8_mult = 0;
    uint32_t query_stride = 0;   // floats between queries (0 = dim): an MRL prefix view searches the first dim_ dimensions of full-length queries
    bool i8_filter = false;
    int bits = 8;
    // two_pass_candidates_device_begin: where this batch leaves its candidate pairs (a parked plan's fallback needs them in _end too)
    u64 *tp_approx = nullptr, *tp_exact = nullptr;
    uint32_t tp_stride = 0;      // entries between queries in both
    int ticket = -1;             // the ticket this search parks in once everything is enqueued (-1: blocking)
    bool nested = false;         // the int8 filter's leftovers on their way through the f16 filter, inside an outer call: never parks
};

struct VectorIndex::BatchedOutcome {
    uint32_t fallbacks = 0;    // queries answered by the exact kernels (int8 two-pass: by its per-query form)
    uint32_t refiltered = 0;   // queries the int8 filter handed to the f16 filter
    bool parked = false;       // enqueued only: the verdicts are read, and both counts known, in _end
};

// What one call fixes for all its rounds: the request, the sample sizes, the workspaces.
struct VectorIndex::BatchedPlan {
    static constexpr uint32_t GMAX = 160;    // queries per pass: 128 (160 opt-in), or 64 for small batches / tails
    static constexpr uint32_t CAPQ = 8192;   // entries one selection pass covers: block lists + pool fit it at the wide shape
    static constexpr uint32_t SPILL = 4096;  // per-query overflow area for candidates that did not fit their block's list
    static constexpr uint32_t KC = kSelectPool;  // approximate candidates re-scored exactly (at most)
    static constexpr uint32_t RA_MAX = 8192;
    BatchedRequest rq;
    // derived
    bool i8f = false, i8 = false, strided = false, skip_b = false, wide_ok = false;
    uint32_t qs = 0;                  // floats between queries
    uint32_t RA = 4096;               // stage A sample rows (dense; <= 8192)
    uint32_t RB = 131072;             // stage B sample rows (upper bound; shrinks with the slab)
    uint32_t ksel_est = 0, ksel = 0;  // the rank the selections anchor on (estimate incl. the int8 filter's growth; exact)
    uint32_t N = 0, QCAP = 0, wide_max = 0, k_eff = 0;
    int wide_pref = 3;
    // per-query verdicts, written by the kernels straight into pinned host memory and read after ONE stream synchronisation
    uint32_t *overflow_all = nullptr, *counts_all = nullptr;
    float *delta = nullptr, *tau = nullptr, *unit = nullptr, *tau_floor = nullptr;
    uint32_t* pool_flag = nullptr;
    u64 *spill = nullptr, *pool = nullptr;
    uint32_t* spill_count = nullptr;
    bool big_pool = false;            // the finish has the second-chance launch: the int8 filter's batches and its leftovers'
};

// One round: up to QCAP queries — the sample stages and every selection are single launches over all its query groups, only the
// main pass is one launch per group.
struct VectorIndex::BatchedRound {
    uint32_t g0 = 0;                  // first query of the round
    int wide_qt = 0, shape = 0, wpb = 0, full_grid = 0, wide_grid = 0;
    uint32_t G = 0, wide_mult = 1, ngroups = 0, QP = 0, ng = 0, tile_rows = 0;
    const float* qg = nullptr;
    uint32_t *overflow = nullptr, *cand_counts = nullptr, *cand_count = nullptr;
    u64* cand = nullptr;
    MfmaScanArgs a{};
    SelectArgs sb{};
    bool anchor = false, short_stages = false;
    int grid_for(uint32_t rows, uint32_t tile) const {
        int g = (int)(((rows + tile - 1) / tile + wpb - 1) / wpb);
        if (g > full_grid) g = full_grid;
        return g < 1 ? 1 : g;
    }
    // one candidate list of `slots` entries per (query, block); 16..32 slots, sized so that lists + pool fit one selection pass
    // when the grid allows (the wide shape's 256 blocks do)
    uint32_t slots_for(int grid) const {
        return std::min<uint32_t>((uint32_t)scan_mfma_max_slots(shape),
                                  std::max<uint32_t>(16, (BatchedPlan::CAPQ - BatchedPlan::KC) / (uint32_t)grid));
    }
};

// A begun search (search_top_k_batched_device_begin / two_pass_candidates_device_begin .. _end).
struct VectorIndex::BatchedTicket {
    enum State : uint8_t { kFree, kParked, kFinishedInBegin } state = kFree;   // parked: all is enqueued, _end reads the verdicts behind `event`
    bool i8f = false;          // the exact search's int8 filter took it: _end keeps the filter's accounts
    uint32_t nq = 0, fallbacks = 0;
    hipEvent_t event = nullptr;   // behind the search's last kernel (created on first use, kept)
    hipStream_t stream = nullptr; // the stream it was enqueued on
    BatchedPlan plan;             // what _end's fallback stage works from
};

}  // namespace fsgpu

#define FSGPU_HIP(expr)                                                   \
    do {                                                                  \
        hipError_t _e = (expr);                                           \
        if (_e != hipSuccess) return ::fsgpu::detail::hip_fail(_e, #expr); \
    } while (0)

#define FSGPU_TRY(expr)            \
    do {                           \
        SearchError _s = (expr);   \
        if (!_s.ok()) return _s;   \
    } while (0)

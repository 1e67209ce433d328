// api_internal.hpp — what the two translation units of the extern "C" boundary share: the handle structs behind the opaque pointers of
// include/fsgpu.h, and the status helpers.  fsgpu_api.cpp holds the product entry points (include/fsgpu.h) and defines everything declared
// here; fsgpu_lab_api.cpp holds the lab ones (include/fsgpu_lab.h).  Private to the library: not installed, nothing here is exported.
#pragma once
#include "../../include/fsgpu.h"

#include <atomic>
#include <exception>
#include <mutex>
#include <new>
#include <shared_mutex>
#include <string>
#include <vector>

#include "bert_embedder.hpp"
#include "bert_reranker.hpp"
#include "coalescer.hpp"
#include "hash_embedder.hpp"
#include "wordpiece.hpp"
#include "index_builder.hpp"
#include "ann_index.hpp"
#include "ivf_index.hpp"
#include "sharded_index.hpp"
#include "vector_index.hpp"
#include "two_tier_index.hpp"

// One in-flight single-item call, parked in a Coalescer until a leader serves it (coalescer.hpp).
struct CoalescedCall : fsgpu::CoalescedRequest {
    fsgpu_status status = FSGPU_OK;
    std::string detail;
};
struct SearchCall : CoalescedCall {
    const float* query = nullptr;
    uint32_t k = 0;
    uint32_t int8_mult = 0;  // 0 = exact search, else search_top_k_int8_two_pass with this multiplier
    const uint64_t* allow = nullptr;  // the caller's allow bitmap (host words): calls that pass the SAME bitmap share a batch
    const uint64_t* allow_dev = nullptr;  // its resident device copy (fsgpu_allow_bitmap), if the caller keeps one
    uint32_t* out_rows = nullptr;
    float* out_scores = nullptr;
    uint32_t* out_count = nullptr;
};
template <class Id>
struct EmbedCall : CoalescedCall {
    const Id* ids = nullptr;
    uint32_t len = 0;
    float* out = nullptr;
};

struct fsgpu_index {
    fsgpu::VectorIndex impl;
    // Lanes (vector_index.hpp): row-level searches from different host threads run on replicas of the index, each behind
    // its own mutex; state_mu is held shared by a search on a replica and exclusively by whatever changes the index
    // (tombstones, WAL, live bitmap, hreduce / variant), which then re-syncs the replicas.
    std::shared_mutex state_mu;
    std::mutex lanes_mu;
    std::atomic<bool> lanes_ready{false};
    std::atomic<uint32_t> lane_rr{0};
    fsgpu::Coalescer<SearchCall> coalescer;
    // leader-only staging (guarded by impl.mutex())
    std::vector<float> co_queries, co_scores;
    std::vector<uint32_t> co_rows, co_counts;
};
struct fsgpu_alignment {
    fsgpu::QualityAlignment impl;
};
struct fsgpu_allow_bitmap {   // a precomputed SearchFilter resident on an index's device
    int device = -1;
    uint64_t nrows = 0, allowed = 0;
    uint64_t generation = 0;       // the index's slab generation it was made for: row ids do not survive compact / vacuum
    std::vector<uint64_t> words;   // host copy: the selectivity rule (1/50) and the coalescer's batch key
    fsgpu::DeviceBuffer dev;
    // the ascending row ids of the set bits, built on the device at first use (fsgpu_search_topk_batched_multi_filtered's
    // selective groups, fsgpu_allow_bitmap_rows) and kept: the handle pins device, record count and generation
    mutable std::mutex rows_mu;
    mutable fsgpu::DeviceBuffer rows;
    mutable bool rows_ready = false;
};
struct fsgpu_sharded {
    fsgpu::ShardedIndex impl;
    // single-query fsgpu_sharded_search calls in flight together ride one batched search of the shards (fsgpu_sharded_set_coalescing)
    fsgpu::Coalescer<SearchCall> coalescer;
    std::vector<float> co_queries, co_scores;   // leader-only staging (guarded by impl.mutex())
    std::vector<uint32_t> co_rows, co_counts;
};
struct fsgpu_m2v {
    fsgpu::Model2VecEmbedder impl;
    fsgpu::Coalescer<EmbedCall<uint32_t>> coalescer;
    std::mutex co_mu;
    std::vector<uint32_t> co_ids, co_offsets;
    std::vector<float> co_out;
};
struct fsgpu_bert {
    fsgpu::NativeEmbedder impl;
    fsgpu::Coalescer<EmbedCall<int32_t>> coalescer;
    std::mutex co_mu;
    std::vector<int32_t> co_ids;
    std::vector<uint32_t> co_offsets;
    std::vector<float> co_out;
};

struct fsgpu_reranker {
    fsgpu::NativeReranker impl;
};
struct fsgpu_index_builder {
    fsgpu::IndexBuilder impl;
};
struct fsgpu_hash {
    fsgpu::HashEmbedder impl;
};
struct fsgpu_wordpiece {
    fsgpu::WordPieceTokenizer impl;
};
struct fsgpu_ann {   // a k-NN table resident on an index's device; searches take the index's locks
    fsgpu::AnnIndex impl;
    fsgpu_index* idx = nullptr;
};
struct fsgpu_ivf {   // centroids and inverted lists resident on an index's device; every call takes the index's locks
    fsgpu::IvfIndex impl;
    fsgpu_index* idx = nullptr;
};

namespace fsgpu {
namespace api __attribute__((visibility("hidden"))) {

// The thread's last-error string (fsgpu_last_error) is ONE object for the whole library, private to fsgpu_api.cpp: every failure, from
// either translation unit, is recorded through these two.
fsgpu_status finish(const SearchError& e);
fsgpu_status fail(fsgpu_status code, const char* detail);

template <typename F>
fsgpu_status guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(FSGPU_ERR_DEVICE, "host allocation failed");
    } catch (const std::exception& ex) {
        return fail(FSGPU_ERR_DEVICE, ex.what());
    } catch (...) {
        return fail(FSGPU_ERR_DEVICE, "unknown exception");
    }
}

// entry points of fsgpu.h whose bodies a lab twin shares (fsgpu_lab_index_query_hubness_topk, fsgpu_lab_wordpiece_encode_stage_ms)
fsgpu_status index_query_hubness(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq, float* out,
                                 float* out_topk);
fsgpu_status wordpiece_encode(fsgpu_wordpiece* tok, WordPieceTokenizer::Request r);

}  // namespace api
}  // namespace fsgpu

// fsgpu_api.cpp — the extern "C" boundary of libfsgpu.so (declared in include/fsgpu.h).
// Plain pointers and sizes only; every entry point catches C++ exceptions and reports a status.
#include "../../include/fsgpu.h"
#include "../../include/fsgpu_lab.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <exception>
#include <limits>
#include <new>
#include <string>
#include <vector>

#include <atomic>
#include <mutex>
#include <shared_mutex>

#include "bert_embedder.hpp"
#include "bert_reranker.hpp"
#include "coalescer.hpp"
#include "hash_embedder.hpp"
#include "wordpiece.hpp"
#include "index_builder.hpp"
#include "ann_index.hpp"
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
namespace {

thread_local std::string g_last_error;

fsgpu_status finish(const fsgpu::SearchError& e) {
    if (!e.ok()) g_last_error = e.detail;
    return e.code;
}

fsgpu_status fail(fsgpu_status code, const char* detail) {
    g_last_error = detail;
    return code;
}

void ann_stats_out(const fsgpu::AnnStats& s, fsgpu_ann_stats* out) {
    out->index_size = s.index_size;
    out->dimension = s.dimension;
    out->ef_search = s.ef_search;
    out->k_requested = s.k_requested;
    out->launches = s.launches;
    out->queries = s.queries;
    out->approximate = s.approximate;
    out->underfilled = s.underfilled;
    out->empty_despite_indexed_points = s.empty_despite_indexed_points;
    out->rows_scored = s.rows_scored;
    out->steps = s.steps;
    out->device_ms = s.device_ms;
}

void certified_out(const fsgpu::CertifiedEf& c, fsgpu_certified_ef* out) {
    out->ef_search = c.ef_search;
    out->meets_target = c.meets_target ? 1u : 0u;
    out->certified_recall = c.certified_recall;
}

template <typename F>
fsgpu_status guarded(F&& body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        return fail(FSGPU_ERR_DEVICE, "host allocation failed");
    } catch (const std::exception& ex) {
        g_last_error = ex.what();
        return FSGPU_ERR_DEVICE;
    } catch (...) {
        return fail(FSGPU_ERR_DEVICE, "unknown exception");
    }
}

// Runs one coalesced batch of single-text embed calls through embed_batch (ids concatenated, offsets rebuilt).
template <class Handle, class Id>
void run_embed_batch(Handle* h, uint32_t dim, std::vector<EmbedCall<Id>*>& batch) {
    std::lock_guard<std::mutex> lock(h->co_mu);
    fsgpu_status st = FSGPU_ERR_DEVICE;
    std::string detail;
    try {
        h->co_ids.clear();
        h->co_offsets.assign(1, 0u);
        for (auto* c : batch) {
            h->co_ids.insert(h->co_ids.end(), c->ids, c->ids + c->len);
            h->co_offsets.push_back((uint32_t)h->co_ids.size());
        }
        h->co_out.resize((size_t)batch.size() * dim);
        fsgpu::SearchError e = h->impl.embed_batch(h->co_ids.data(), h->co_offsets.data(), (uint32_t)batch.size(), h->co_out.data());
        st = e.code;
        detail = e.detail;
    } catch (const std::exception& ex) {
        detail = ex.what();
    } catch (...) {
        detail = "unknown exception";
    }
    for (size_t i = 0; i < batch.size(); ++i) {
        batch[i]->status = st;
        batch[i]->detail = detail;
        if (st == FSGPU_OK) std::memcpy(batch[i]->out, h->co_out.data() + i * dim, (size_t)dim * 4);
    }
}

// One single-query call parked in the index's coalescer: concurrent callers ride one batched pass (results are
// bit-identical to the direct path).  int8_mult 0 = exact search, else the int8 two-pass with that multiplier.
fsgpu_status coalesced_search(fsgpu_index* idx, const float* query, uint32_t k, uint32_t int8_mult, uint32_t* out_rows,
                              float* out_scores, uint32_t* out_count, const uint64_t* allow = nullptr, const uint64_t* allow_dev = nullptr) {
    return guarded([&]() -> fsgpu_status {
        SearchCall call;
        call.query = query;
        call.k = k;
        call.int8_mult = int8_mult;
        call.allow = allow;
        call.allow_dev = allow_dev;
        call.out_rows = out_rows;
        call.out_scores = out_scores;
        call.out_count = out_count;
        idx->coalescer.submit(
            &call,
            [idx](std::vector<SearchCall*>& batch) {
                std::lock_guard<std::mutex> lock(idx->impl.mutex());
                const uint32_t n = (uint32_t)batch.size(), dim = idx->impl.dimension(), kk = batch[0]->k;
                const uint32_t mult = batch[0]->int8_mult;
                const uint64_t* allow_bm = batch[0]->allow;   // one filter for the whole batch (compatible() below)
                const uint64_t* allow_res = batch[0]->allow_dev;
                fsgpu_status st = FSGPU_ERR_DEVICE;
                std::string detail;
                try {
                    idx->co_queries.resize((size_t)n * dim);
                    idx->co_rows.resize((size_t)n * kk);
                    idx->co_scores.resize((size_t)n * kk);
                    idx->co_counts.resize(n);
                    for (uint32_t i = 0; i < n; ++i)
                        std::memcpy(idx->co_queries.data() + (size_t)i * dim, batch[i]->query, (size_t)dim * 4);
                    uint32_t fb = 0;
                    fsgpu::SearchError e;
                    if (mult) {
                        e = idx->impl.search_top_k_int8_batched(idx->co_queries.data(), n, dim, kk, mult, idx->co_rows.data(),
                                                                idx->co_scores.data(), idx->co_counts.data(), &fb);
                    } else if (n <= 4) {
                        // up to four callers: one pass of the exact multi-query kernel is quicker than the staged
                        // matrix-core pipeline; beyond that the batched path serves 128 and more per pass
                        e = idx->impl.search_top_k(idx->co_queries.data(), n, dim, kk, allow_bm, idx->co_rows.data(),
                                                   idx->co_scores.data(), idx->co_counts.data(), allow_res);
                    } else {
                        e = idx->impl.search_top_k_batched(idx->co_queries.data(), n, dim, kk, allow_bm, idx->co_rows.data(),
                                                           idx->co_scores.data(), idx->co_counts.data(), &fb, allow_res);
                    }
                    st = e.code;
                    detail = e.detail;
                } catch (const std::exception& ex) {
                    detail = ex.what();
                } catch (...) {
                    detail = "unknown exception";
                }
                for (uint32_t i = 0; i < n; ++i) {
                    batch[i]->status = st;
                    batch[i]->detail = detail;
                    if (st != FSGPU_OK) continue;
                    std::memcpy(batch[i]->out_rows, idx->co_rows.data() + (size_t)i * kk, (size_t)kk * 4);
                    std::memcpy(batch[i]->out_scores, idx->co_scores.data() + (size_t)i * kk, (size_t)kk * 4);
                    *batch[i]->out_count = idx->co_counts[i];
                }
            },
            [](const SearchCall& a, const SearchCall& b) { return a.k == b.k && a.int8_mult == b.int8_mult && a.allow == b.allow; });
        if (call.exec_threw) return fail(FSGPU_ERR_DEVICE, "coalesced batch failed before this request was served");
        if (call.status != FSGPU_OK) g_last_error = call.detail;
        return call.status;
    });
}

// The sharded twin of coalesced_search: one single-query request (exact, or the int8 two-pass with call.int8_mult) parked in the
// handle's coalescer; the leader runs ONE search of the shards for the whole batch — more than four exact callers take the
// matrix-core batched mode, whose rows and score bits are the exact kernels' — and hands every caller its own hits.
fsgpu_status coalesced_sharded_search(fsgpu_sharded* idx, const float* query, uint32_t query_len, uint32_t k, uint32_t int8_mult,
                                      uint32_t* out_rows, float* out_scores, uint32_t* out_count) {
    return guarded([&]() -> fsgpu_status {
        SearchCall call;
        call.query = query;
        call.k = k;
        call.int8_mult = int8_mult;
        call.out_rows = out_rows;
        call.out_scores = out_scores;
        call.out_count = out_count;
        idx->coalescer.submit(
            &call,
            [idx, query_len](std::vector<SearchCall*>& batch) {
                std::lock_guard<std::mutex> lock(idx->impl.mutex());
                const uint32_t n = (uint32_t)batch.size(), dim = idx->impl.dimension(), kk = batch[0]->k;
                fsgpu_status st = FSGPU_ERR_DEVICE;
                std::string detail;
                try {
                    idx->co_queries.resize((size_t)n * dim);
                    idx->co_rows.resize((size_t)n * kk);
                    idx->co_scores.resize((size_t)n * kk);
                    idx->co_counts.resize(n);
                    for (uint32_t i = 0; i < n; ++i)
                        std::memcpy(idx->co_queries.data() + (size_t)i * dim, batch[i]->query, (size_t)dim * 4);
                    fsgpu::ShardedIndex::Request rq;
                    rq.queries = idx->co_queries.data();
                    rq.nq = n;
                    rq.k = kk;
                    rq.multiplier = batch[0]->int8_mult;
                    rq.mode = batch[0]->int8_mult ? fsgpu::ShardedIndex::kInt8TwoPass
                              : n <= 4            ? fsgpu::ShardedIndex::kExact
                                                  : fsgpu::ShardedIndex::kBatched;
                    const fsgpu::SearchError e =
                        idx->impl.search(rq, query_len, idx->co_rows.data(), idx->co_scores.data(), idx->co_counts.data(), nullptr);
                    st = e.code;
                    detail = e.detail;
                } catch (const std::exception& ex) {
                    detail = ex.what();
                } catch (...) {
                    detail = "unknown exception";
                }
                for (uint32_t i = 0; i < n; ++i) {
                    batch[i]->status = st;
                    batch[i]->detail = detail;
                    if (st != FSGPU_OK) continue;
                    std::memcpy(batch[i]->out_rows, idx->co_rows.data() + (size_t)i * kk, (size_t)kk * 4);
                    std::memcpy(batch[i]->out_scores, idx->co_scores.data() + (size_t)i * kk, (size_t)kk * 4);
                    *batch[i]->out_count = idx->co_counts[i];
                }
            },
            [](const SearchCall& a, const SearchCall& b) { return a.k == b.k && a.int8_mult == b.int8_mult; });
        if (call.exec_threw) return fail(FSGPU_ERR_DEVICE, "coalesced batch failed before this request was served");
        if (call.status != FSGPU_OK) g_last_error = call.detail;
        return call.status;
    });
}

// compact / vacuum: the state lock exclusively — a search holds it shared for as long as it is on a lane, so none is —, the index's
// lock, and every replica's lock taken once so that whatever held it has left (they cannot be held across the call: a rewrite destroys
// the replicas).  The lanes are made again on demand.
template <typename F>
fsgpu_status rewrite_locked(fsgpu_index* idx, F&& body) {
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lanes(idx->lanes_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        for (size_t i = 0; i < idx->impl.replica_count(); ++i) std::lock_guard<std::mutex> drained(idx->impl.replica(i)->mutex());
        const uint64_t before = idx->impl.generation();
        const fsgpu::SearchError e = body();
        if (idx->impl.generation() != before) idx->lanes_ready.store(false, std::memory_order_release);
        return finish(e);
    });
}

}  // namespace

extern "C" {

const char* fsgpu_version(void) { return "fsgpu 0.1.0 (gfx950)"; }

int32_t fsgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* fsgpu_last_error(void) { return g_last_error.c_str(); }

const char* fsgpu_last_main_pass_kernel(void) { return fsgpu::last_main_pass_kernel(); }

fsgpu_status fsgpu_index_create(int32_t device, uint32_t dim, uint64_t nrows, const void* slab_f16_le,
                                const uint64_t* live_bitmap, uint64_t row_base, fsgpu_index** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_index();
        fsgpu::SearchError e = h->impl.init_host(device, dim, nrows, slab_f16_le, live_bitmap, row_base);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_index_create_device(int32_t device, uint32_t dim, uint64_t nrows, const void* slab_f16_dev,
                                       const uint64_t* live_bitmap_dev, uint64_t row_base, fsgpu_index** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_index();
        fsgpu::SearchError e = h->impl.init_device(device, dim, nrows, slab_f16_dev, live_bitmap_dev, row_base);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_index_create_f32(int32_t device, uint32_t dim, uint64_t nrows, const void* slab_f32_le,
                                    const uint64_t* live_bitmap, uint64_t row_base, fsgpu_index** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_index();
        fsgpu::SearchError e = h->impl.init_host(device, dim, nrows, slab_f32_le, live_bitmap, row_base, true);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_index_create_f32_device(int32_t device, uint32_t dim, uint64_t nrows, const void* slab_f32_dev,
                                           const uint64_t* live_bitmap_dev, uint64_t row_base, fsgpu_index** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_index();
        fsgpu::SearchError e = h->impl.init_device(device, dim, nrows, slab_f32_dev, live_bitmap_dev, row_base, true);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_index_open_fsvi(const char* path, int32_t device, fsgpu_index** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_index();
        fsgpu::SearchError e = h->impl.open_fsvi(path, device);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

void fsgpu_index_destroy(fsgpu_index* idx) { delete idx; }

uint64_t fsgpu_index_record_count(const fsgpu_index* idx) { return idx ? idx->impl.record_count() : 0; }
uint32_t fsgpu_index_dimension(const fsgpu_index* idx) { return idx ? idx->impl.dimension() : 0; }

fsgpu_status fsgpu_index_set_hreduce(fsgpu_index* idx, int32_t mode) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (mode < FSGPU_HREDUCE_SSE2 || mode > FSGPU_HREDUCE_SEQ) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown hreduce mode");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.hreduce = mode;
    idx->impl.sync_replicas();
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_batched_filter(fsgpu_index* idx, int32_t filter) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (filter < FSGPU_FILTER_AUTO || filter > FSGPU_FILTER_INT8) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown batched filter");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.batched_filter = filter;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_filter_rotation(fsgpu_index* idx, int32_t mode) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (mode < FSGPU_ROTATION_AUTO || mode > FSGPU_ROTATION_ON) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown rotation mode");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.filter_rotation = mode;
    return FSGPU_OK;
}

int32_t fsgpu_index_filter_rotated(fsgpu_index* idx) {
    if (!idx) return 0;
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    return idx->impl.filter_rotated() ? 1 : 0;
}

fsgpu_status fsgpu_index_set_int8_latency(fsgpu_index* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.int8_latency = enabled != 0;
    idx->impl.int8_latency_build_now = enabled == FSGPU_INT8_LATENCY_BUILD_NOW;
    if (enabled == FSGPU_INT8_LATENCY_BUILD_NOW) return finish(idx->impl.prepare_int8_latency());
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_batched_filter_stats(fsgpu_index* idx, uint64_t* int8_queries, uint64_t* refiltered_f16,
                                              int32_t* int8_active) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    if (int8_queries) *int8_queries = idx->impl.i8f_queries;
    if (refiltered_f16) *refiltered_f16 = idx->impl.i8f_refiltered;
    if (int8_active) *int8_active = idx->impl.int8_filter_active() ? 1 : 0;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_int8_filter_bound(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, float* out_delta,
                                           float* out_query_scale, float* out_slab_scale, int8_t* out_queries_i8, int8_t* out_slab_i8) {
    if (!idx || (nq && !queries)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.int8_filter_bound(queries, nq, query_len, out_delta, out_query_scale, out_slab_scale, out_queries_i8,
                                                  out_slab_i8));
    });
}

fsgpu_status fsgpu_index_doc_id(const fsgpu_index* idx, uint32_t row, const char** ptr, uint32_t* len) {
    if (!idx || !ptr || !len) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return finish(idx->impl.doc_id_at(row, ptr, len));
}

fsgpu_status fsgpu_index_soft_delete(fsgpu_index* idx, const char* doc_id, uint32_t doc_id_len, int32_t* deleted) {
    if (!idx || !doc_id || !deleted) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const fsgpu::SearchError e = idx->impl.soft_delete(doc_id, doc_id_len, deleted);
        idx->impl.sync_replicas();   // the live bitmap may have been re-uploaded
        return finish(e);
    });
}

fsgpu_status fsgpu_index_allow_bitmap_for_hashes(const fsgpu_index* idx, const uint64_t* hashes, uint32_t n,
                                                 uint64_t* allow_bitmap_out, uint64_t* rows_matched) {
    if (!idx || (!hashes && n) || !allow_bitmap_out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(const_cast<fsgpu_index*>(idx)->impl.mutex());
        return finish(idx->impl.allow_bitmap_for_hashes(hashes, n, allow_bitmap_out, rows_matched));
    });
}

fsgpu_status fsgpu_index_set_live_bitmap(fsgpu_index* idx, const uint64_t* live_bitmap) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const fsgpu::SearchError e = idx->impl.set_live_bitmap(live_bitmap);
        idx->impl.sync_replicas();
        return finish(e);
    });
}

static fsgpu_status search_topk_common(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                       const uint64_t* allow_bitmap, const uint64_t* allow_resident_dev, uint32_t* out_rows,
                                       float* out_scores, uint32_t* out_counts, bool exact_only = false) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (!exact_only && idx->coalescer.enabled() && nq == 1 && k >= 1 && k <= 64 && query_len == idx->impl.dimension())
        return coalesced_search(idx, queries, k, 0, out_rows, out_scores, out_counts, allow_bitmap, allow_resident_dev);
    return guarded([&]() -> fsgpu_status {
        // this index if it is free, else a free replica, else queue on one of the lanes in turn
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::unique_lock<std::mutex> lock(idx->impl.mutex(), std::try_to_lock);
        fsgpu::VectorIndex* lane = &idx->impl;
        if (!lock.owns_lock()) {
            if (!idx->lanes_ready.load(std::memory_order_acquire)) {
                std::lock_guard<std::mutex> init(idx->lanes_mu);
                if (!idx->lanes_ready.load(std::memory_order_relaxed)) {
                    std::lock_guard<std::mutex> primary(idx->impl.mutex());   // the replicas copy the primary's state
                    fsgpu::SearchError e = idx->impl.ensure_replicas();
                    if (!e.ok()) return finish(e);
                    idx->lanes_ready.store(true, std::memory_order_release);
                }
            }
            const size_t n = idx->impl.replica_count();
            for (size_t i = 0; i < n && !lock.owns_lock(); ++i) {
                lock = std::unique_lock<std::mutex>(idx->impl.replica(i)->mutex(), std::try_to_lock);
                if (lock.owns_lock()) lane = idx->impl.replica(i);
            }
            if (!lock.owns_lock()) {
                const uint32_t pick = idx->lane_rr.fetch_add(1, std::memory_order_relaxed) % (uint32_t)(n + 1);
                lane = pick == 0 ? &idx->impl : idx->impl.replica(pick - 1);
                lock = std::unique_lock<std::mutex>(lane->mutex());
            }
        }
        lane->exact_only_ = exact_only;   // (under the lane's mutex)
        const fsgpu::SearchError e = lane->search_top_k(queries, nq, query_len, k, allow_bitmap, out_rows, out_scores, out_counts, allow_resident_dev);
        lane->exact_only_ = false;
        return finish(e);
    });
}

fsgpu_status fsgpu_search_topk_exact(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                     const uint64_t* allow_bitmap, uint32_t* out_rows, float* out_scores, uint32_t* out_counts) {
    return search_topk_common(idx, queries, nq, query_len, k, allow_bitmap, nullptr, out_rows, out_scores, out_counts, true);
}

fsgpu_status fsgpu_search_topk(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                               const uint64_t* allow_bitmap, uint32_t* out_rows, float* out_scores,
                               uint32_t* out_counts) {
    return search_topk_common(idx, queries, nq, query_len, k, allow_bitmap, nullptr, out_rows, out_scores, out_counts);
}

// ---- resident filters: a precomputed SearchFilter uploaded once and reused (filter.rs:19-56; search.rs:1114-1255) ----
fsgpu_status fsgpu_allow_bitmap_create(fsgpu_index* idx, const uint64_t* allow_bitmap, fsgpu_allow_bitmap** out) {
    if (!idx || !allow_bitmap || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto f = std::make_unique<fsgpu_allow_bitmap>();
        f->device = idx->impl.device();
        f->nrows = idx->impl.record_count();
        f->generation = idx->impl.generation();
        const size_t words = (size_t)((f->nrows + 63) / 64);
        f->words.assign(allow_bitmap, allow_bitmap + words);
        if (words && (f->nrows & 63)) f->words.back() &= (1ull << (f->nrows & 63)) - 1ull;
        for (uint64_t w : f->words) f->allowed += (uint64_t)__builtin_popcountll(w);
        if (f->device < 0) return fail(FSGPU_ERR_NO_DEVICE, "index has no device");
        if (hipSetDevice(f->device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        fsgpu::SearchError e = f->dev.reserve(std::max<size_t>(words, 1) * 8);
        if (!e.ok()) return finish(e);
        if (words && hipMemcpy(f->dev.ptr, f->words.data(), words * 8, hipMemcpyHostToDevice) != hipSuccess) {
            f->dev.release();
            return fail(FSGPU_ERR_DEVICE, "upload of the allow bitmap failed");
        }
        *out = f.release();
        return FSGPU_OK;
    });
}

void fsgpu_allow_bitmap_destroy(fsgpu_allow_bitmap* f) {
    if (!f) return;
    if (f->device >= 0) (void)hipSetDevice(f->device);
    f->dev.release();
    f->rows.release();
    delete f;
}

uint64_t fsgpu_allow_bitmap_allowed_rows(const fsgpu_allow_bitmap* f) { return f ? f->allowed : 0; }

static fsgpu_status check_filter(const fsgpu_index* idx, const fsgpu_allow_bitmap* f) {
    if (!idx || !f) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (f->device != idx->impl.device() || f->nrows != idx->impl.record_count())
        return fail(FSGPU_ERR_INVALID_CONFIG, "the allow bitmap was made for another index (device or record count differ)");
    if (f->generation != idx->impl.generation())   // (a vacuum followed by appends can restore the old record count)
        return fail(FSGPU_ERR_INVALID_CONFIG, "the allow bitmap was made before the index was compacted or vacuumed: its row ids are stale");
    return FSGPU_OK;
}

fsgpu_status fsgpu_search_topk_filtered(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                        const fsgpu_allow_bitmap* filter, uint32_t* out_rows, float* out_scores, uint32_t* out_counts) {
    const fsgpu_status c = check_filter(idx, filter);
    if (c != FSGPU_OK) return c;
    return search_topk_common(idx, queries, nq, query_len, k, filter->words.data(), static_cast<const uint64_t*>(filter->dev.ptr), out_rows,
                              out_scores, out_counts);
}

fsgpu_status fsgpu_search_topk_batched_filtered(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                const fsgpu_allow_bitmap* filter, uint32_t* out_rows, float* out_scores,
                                                uint32_t* out_counts, uint32_t* out_fallbacks) {
    const fsgpu_status c = check_filter(idx, filter);
    if (c != FSGPU_OK) return c;
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_batched(queries, nq, query_len, k, filter->words.data(), out_rows, out_scores, out_counts,
                                                     out_fallbacks, static_cast<const uint64_t*>(filter->dev.ptr)));
    });
}

// ---- a filter per query (vector_index_filtered.cpp) ----
// the handle's row list, built on first use
static fsgpu_status ensure_filter_rows(const fsgpu_allow_bitmap* f) {
    std::lock_guard<std::mutex> lock(f->rows_mu);
    if (f->rows_ready) return FSGPU_OK;
    const fsgpu::SearchError e = fsgpu::build_filter_row_list(f->device, static_cast<const uint64_t*>(f->dev.ptr), f->nrows, f->allowed, &f->rows);
    if (!e.ok()) return finish(e);
    f->rows_ready = true;
    return FSGPU_OK;
}

fsgpu_status fsgpu_allow_bitmap_rows(const fsgpu_allow_bitmap* filter, uint32_t* out_rows, uint64_t cap, uint64_t* out_n) {
    if (!filter || !out_n || (cap && !out_rows)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        *out_n = filter->allowed;
        const fsgpu_status c = ensure_filter_rows(filter);
        if (c != FSGPU_OK) return c;
        const uint64_t n = std::min<uint64_t>(cap, filter->allowed);
        if (n == 0) return FSGPU_OK;
        if (hipSetDevice(filter->device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        if (hipMemcpy(out_rows, filter->rows.ptr, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess)
            return fail(FSGPU_ERR_DEVICE, "download of the row list failed");
        return FSGPU_OK;
    });
}

// Everything that can be refused is refused here, before anything is launched; the views of the filters for the index.
static fsgpu_status multi_filter_views(const fsgpu_index* idx, uint32_t nq, uint32_t query_len, const fsgpu_allow_bitmap* const* filters,
                                       uint32_t nfilters, const int32_t* filter_of_query, std::vector<fsgpu::ResidentFilterView>* views) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if ((nfilters && !filters) || (nq && !filter_of_query)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (query_len != idx->impl.dimension())
        return fail(FSGPU_ERR_DIMENSION_MISMATCH, ("expected " + std::to_string(idx->impl.dimension()) + ", found " + std::to_string(query_len)).c_str());
    for (uint32_t f = 0; f < nfilters; ++f) {
        const fsgpu_status c = check_filter(idx, filters[f]);
        if (c != FSGPU_OK) return c;
    }
    const fsgpu::SearchError e = fsgpu::multi_filter_plan(idx->impl.record_count(), nullptr, nfilters, filter_of_query, nq, nullptr, nullptr,
                                                          nullptr, nullptr);
    if (!e.ok()) return finish(e);
    std::vector<uint8_t> named(nfilters, 0);
    for (uint32_t q = 0; q < nq; ++q)
        if (filter_of_query[q] >= 0) named[filter_of_query[q]] = 1;
    views->resize(nfilters);
    const uint64_t nrows = idx->impl.record_count();
    for (uint32_t f = 0; f < nfilters; ++f) {
        fsgpu::ResidentFilterView& v = (*views)[f];
        v.words_host = filters[f]->words.data();
        v.words_dev = static_cast<const uint64_t*>(filters[f]->dev.ptr);
        v.allowed = filters[f]->allowed;
        // a selective filter some query names: its row list (first use builds it, on the device)
        if (named[f] && v.allowed && (unsigned __int128)v.allowed * 50u < (unsigned __int128)nrows) {
            const fsgpu_status c = ensure_filter_rows(filters[f]);
            if (c != FSGPU_OK) return c;
            v.rows_dev = static_cast<const uint32_t*>(filters[f]->rows.ptr);
        }
    }
    return FSGPU_OK;
}

fsgpu_status fsgpu_search_topk_batched_multi_filtered(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                      const fsgpu_allow_bitmap* const* filters, uint32_t nfilters,
                                                      const int32_t* filter_of_query, uint32_t* out_rows, float* out_scores,
                                                      uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (out_fallbacks) *out_fallbacks = 0;
    if (idx && nq && (!queries || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::ResidentFilterView> views;
        const fsgpu_status c = multi_filter_views(idx, nq, query_len, filters, nfilters, filter_of_query, &views);
        if (c != FSGPU_OK) return c;
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_multi_filtered_host(queries, nq, query_len, k, views.data(), nfilters, filter_of_query, out_rows,
                                                                 out_scores, out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_search_topk_batched_multi_filtered_device_queries(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                                     uint32_t k, const fsgpu_allow_bitmap* const* filters, uint32_t nfilters,
                                                                     const int32_t* filter_of_query, uint32_t* out_rows_dev,
                                                                     float* out_scores_dev, uint32_t* out_counts_dev, void* hip_stream,
                                                                     uint32_t* out_fallbacks) {
    if (out_fallbacks) *out_fallbacks = 0;
    if (idx && nq && (!queries_dev || !out_counts_dev || (k && (!out_rows_dev || !out_scores_dev))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::ResidentFilterView> views;
        const fsgpu_status c = multi_filter_views(idx, nq, query_len, filters, nfilters, filter_of_query, &views);
        if (c != FSGPU_OK) return c;
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_multi_filtered(queries_dev, nq, query_len, k, views.data(), nfilters, filter_of_query, out_rows_dev,
                                                            out_scores_dev, out_counts_dev, static_cast<hipStream_t>(hip_stream), out_fallbacks));
    });
}

fsgpu_status fsgpu_index_multi_filter_stats(fsgpu_index* idx, uint64_t* gathered, uint64_t* scanned, uint64_t* unfiltered, uint64_t* fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    if (gathered) *gathered = idx->impl.multi_gathered;
    if (scanned) *scanned = idx->impl.multi_scanned;
    if (unfiltered) *unfiltered = idx->impl.multi_unfiltered;
    if (fallbacks) *fallbacks = idx->impl.multi_fallbacks;
    return FSGPU_OK;
}

fsgpu_status fsgpu_lab_multi_filter_plan(uint64_t nrows, const uint64_t* allowed_per_filter, uint32_t nfilters, const int32_t* filter_of_query,
                                         uint32_t nq, int32_t* out_group_of_query, int32_t* out_path_of_group, uint32_t* out_ngroups) {
    if ((nfilters && !allowed_per_filter) || (nq && (!filter_of_query || !out_group_of_query || !out_path_of_group)) || !out_ngroups)
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        return finish(fsgpu::multi_filter_plan(nrows, allowed_per_filter, nfilters, filter_of_query, nq, out_group_of_query, out_path_of_group,
                                               nullptr, out_ngroups));
    });
}

fsgpu_status fsgpu_index_set_coalescing(fsgpu_index* idx, uint32_t max_batch, uint32_t max_wait_us) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    idx->coalescer.configure(max_batch, max_wait_us);
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_coalescing_stats(fsgpu_index* idx, uint64_t* batches, uint64_t* requests) {
    if (!idx || !batches || !requests) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    idx->coalescer.stats(batches, requests);
    return FSGPU_OK;
}

fsgpu_status fsgpu_search_topk_device(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                      uint32_t k, const uint64_t* allow_bitmap_dev, uint32_t* out_rows_dev,
                                      float* out_scores_dev, uint32_t* out_counts_dev, void* hip_stream) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries_dev || !out_counts_dev || (k && (!out_rows_dev || !out_scores_dev))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_device(queries_dev, nq, query_len, k, allow_bitmap_dev, out_rows_dev,
                                                    out_scores_dev, out_counts_dev,
                                                    static_cast<hipStream_t>(hip_stream)));
    });
}

fsgpu_status fsgpu_search_topk_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len,
                                       uint32_t k, const uint64_t* allow_bitmap, uint32_t* out_rows, float* out_scores,
                                       uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_batched(queries, nq, query_len, k, allow_bitmap, out_rows, out_scores,
                                                     out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_search_topk_batched_device(fsgpu_index* idx, const float* queries_dev, uint32_t nq,
                                              uint32_t query_len, uint32_t k, const uint64_t* allow_bitmap_dev,
                                              uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                              void* hip_stream, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries_dev || !out_counts_dev || (k && (!out_rows_dev || !out_scores_dev))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        if (k == 0 || idx->impl.record_count() == 0) {
            if (hipMemsetAsync(out_counts_dev, 0, (size_t)nq * 4, static_cast<hipStream_t>(hip_stream)) != hipSuccess)
                return fail(FSGPU_ERR_DEVICE, "hipMemsetAsync failed");
            return FSGPU_OK;
        }
        return finish(idx->impl.search_top_k_batched_device(queries_dev, nq, query_len, k, allow_bitmap_dev, out_rows_dev,
                                                            out_scores_dev, out_counts_dev,
                                                            static_cast<hipStream_t>(hip_stream), out_fallbacks));
    });
}

fsgpu_status fsgpu_search_topk_batched_packed_device(fsgpu_index* idx, const float* queries_dev, uint32_t nq,
                                                     uint32_t query_len, uint32_t k, const uint64_t* allow_bitmap_dev,
                                                     uint64_t* out_packed_dev, void* hip_stream, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && k && (!queries_dev || !out_packed_dev)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (k > 256) return fail(FSGPU_ERR_INVALID_CONFIG, "packed shard search supports k <= 256");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        if (nq == 0 || k == 0) return FSGPU_OK;
        if (idx->impl.record_count() == 0) {
            if (hipMemsetAsync(out_packed_dev, 0xff, (size_t)nq * k * 8, static_cast<hipStream_t>(hip_stream)) != hipSuccess)
                return fail(FSGPU_ERR_DEVICE, "hipMemsetAsync failed");
            return FSGPU_OK;
        }
        return finish(idx->impl.search_top_k_batched_device(queries_dev, nq, query_len, k, allow_bitmap_dev, nullptr,
                                                            nullptr, nullptr, static_cast<hipStream_t>(hip_stream),
                                                            out_fallbacks, out_packed_dev));
    });
}

fsgpu_status fsgpu_search_topk_batched_device_begin(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                                    const uint64_t* allow_bitmap_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                                                    uint32_t* out_counts_dev, uint64_t* out_packed_dev, void* hip_stream, int32_t* out_ticket) {
    if (!idx || !out_ticket) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (nq == 0 || k == 0 || !queries_dev) return fail(FSGPU_ERR_INVALID_CONFIG, "a begun search needs queries and k >= 1");
    if (out_packed_dev && k > 256) return fail(FSGPU_ERR_INVALID_CONFIG, "packed shard search supports k <= 256");
    if (!out_packed_dev && !(out_rows_dev && out_scores_dev && out_counts_dev)) return fail(FSGPU_ERR_NULL_ARGUMENT, "no output");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        if (idx->impl.record_count() == 0) return fail(FSGPU_ERR_INVALID_CONFIG, "the index is empty: use the blocking form");
        return finish(idx->impl.search_top_k_batched_device_begin(queries_dev, nq, query_len, k, allow_bitmap_dev, out_rows_dev, out_scores_dev,
                                                                  out_counts_dev, static_cast<hipStream_t>(hip_stream), out_packed_dev, out_ticket));
    });
}

fsgpu_status fsgpu_search_topk_batched_device_end(fsgpu_index* idx, int32_t ticket, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_batched_device_end(ticket, out_fallbacks));
    });
}

fsgpu_status fsgpu_search_topk_batched_device_end_late(fsgpu_index* idx, int32_t ticket, uint32_t* out_fallbacks, uint32_t* out_late_answers) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_batched_device_end(ticket, out_fallbacks, out_late_answers));
    });
}

fsgpu_status fsgpu_search_topk_packed_device(fsgpu_index* idx, const float* queries_dev, uint32_t nq,
                                             uint32_t query_len, uint32_t k, const uint64_t* allow_bitmap_dev,
                                             uint64_t* out_packed_dev, void* hip_stream) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && k && (!queries_dev || !out_packed_dev)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_packed_device(queries_dev, nq, query_len, k, allow_bitmap_dev,
                                                           out_packed_dev, static_cast<hipStream_t>(hip_stream)));
    });
}

fsgpu_status fsgpu_merge_topk_device(int32_t device, const uint64_t* lists_dev, uint32_t nq, uint32_t nlists,
                                     uint32_t list_len, uint64_t q_stride, uint64_t l_stride, uint32_t k,
                                     uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                     void* hip_stream) {
    if (nq && (!lists_dev || !out_rows_dev || !out_scores_dev || !out_counts_dev))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (k == 0 || k > 1024) return fail(FSGPU_ERR_INVALID_CONFIG, "merge supports 1 <= k <= 1024");
    return guarded([&]() -> fsgpu_status {
        return finish(fsgpu::merge_packed_lists_device(device, lists_dev, nq, nlists, list_len, q_stride, l_stride, k,
                                                       out_rows_dev, out_scores_dev, out_counts_dev,
                                                       static_cast<hipStream_t>(hip_stream)));
    });
}

// search_top_k_classified (crates/frankensearch-index/src/search.rs:227-261)
// ---- row-sharded index: one handle, one call per search (sharded_index.cpp) ----
fsgpu_status fsgpu_sharded_create_grouped(const int32_t* devices, uint32_t ndev, uint32_t query_groups, uint32_t dim, uint64_t nrows,
                                          const void* slab_f16_le, const uint64_t* live_bitmap, int32_t exchange, fsgpu_sharded** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_sharded();
        fsgpu::SearchError e = h->impl.init_host(devices, ndev, dim, nrows, slab_f16_le, live_bitmap, exchange, query_groups);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_sharded_create(const int32_t* devices, uint32_t ndev, uint32_t dim, uint64_t nrows, const void* slab_f16_le,
                                  const uint64_t* live_bitmap, int32_t exchange, fsgpu_sharded** out) {
    return fsgpu_sharded_create_grouped(devices, ndev, 1, dim, nrows, slab_f16_le, live_bitmap, exchange, out);
}

fsgpu_status fsgpu_sharded_create_device_grouped(const int32_t* devices, uint32_t ndev, uint32_t query_groups, uint32_t dim,
                                                 const uint64_t* shard_rows, const void* const* shard_slabs_dev,
                                                 const uint64_t* const* shard_live_dev, int32_t exchange, fsgpu_sharded** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_sharded();
        fsgpu::SearchError e = h->impl.init_device(devices, ndev, dim, shard_rows, shard_slabs_dev, shard_live_dev, exchange, query_groups);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_sharded_create_device(const int32_t* devices, uint32_t ndev, uint32_t dim, const uint64_t* shard_rows,
                                         const void* const* shard_slabs_dev, const uint64_t* const* shard_live_dev,
                                         int32_t exchange, fsgpu_sharded** out) {
    return fsgpu_sharded_create_device_grouped(devices, ndev, 1, dim, shard_rows, shard_slabs_dev, shard_live_dev, exchange, out);
}

uint32_t fsgpu_sharded_query_groups(const fsgpu_sharded* idx) { return idx ? idx->impl.query_groups() : 0; }
uint32_t fsgpu_sharded_row_shards(const fsgpu_sharded* idx) { return idx ? idx->impl.row_shards() : 0; }

fsgpu_status fsgpu_sharded_set_int8_latency(fsgpu_sharded* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.set_int8_latency(enabled != 0));
    });
}

void fsgpu_sharded_destroy(fsgpu_sharded* idx) { delete idx; }
uint64_t fsgpu_sharded_record_count(const fsgpu_sharded* idx) { return idx ? idx->impl.record_count() : 0; }
uint32_t fsgpu_sharded_dimension(const fsgpu_sharded* idx) { return idx ? idx->impl.dimension() : 0; }
uint32_t fsgpu_sharded_shard_count(const fsgpu_sharded* idx) { return idx ? idx->impl.shard_count() : 0; }
int32_t fsgpu_sharded_exchange_mode(const fsgpu_sharded* idx) { return idx ? idx->impl.exchange_mode() : 0; }
int32_t fsgpu_sharded_device(const fsgpu_sharded* idx, uint32_t shard) { return idx ? idx->impl.shard_device(shard) : -1; }

fsgpu_status fsgpu_sharded_shard_range(const fsgpu_sharded* idx, uint32_t shard, uint64_t* row_lo, uint64_t* row_hi) {
    if (!idx || !row_lo || !row_hi) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (!idx->impl.shard_range(shard, row_lo, row_hi)) return fail(FSGPU_ERR_INVALID_CONFIG, "shard ordinal out of range");
    return FSGPU_OK;
}

fsgpu_status fsgpu_sharded_set_hreduce(fsgpu_sharded* idx, int32_t mode) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (mode < FSGPU_HREDUCE_SSE2 || mode > FSGPU_HREDUCE_SEQ) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown hreduce mode");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.set_hreduce(mode);
    return FSGPU_OK;
}

static fsgpu::ShardedIndex::Request sharded_request(const fsgpu_sharded_request* rq) {
    fsgpu::ShardedIndex::Request r;
    r.queries = rq->queries;
    r.queries_dev = rq->queries_dev;
    r.nq = rq->nq;
    r.k = rq->k;
    r.mode = static_cast<fsgpu::ShardedIndex::Mode>(rq->mode);
    r.multiplier = rq->candidate_multiplier;
    r.allow = rq->allow_bitmap;
    return r;
}

static fsgpu_status check_sharded_request(const fsgpu_sharded* idx, const fsgpu_sharded_request* rq) {
    if (!idx || !rq) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (rq->nq && !rq->queries && !rq->queries_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "queries is null");
    if (rq->mode < FSGPU_SHARDED_EXACT || rq->mode > FSGPU_SHARDED_4BIT_TWO_PASS) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown search mode");
    return FSGPU_OK;
}

fsgpu_status fsgpu_sharded_search(fsgpu_sharded* idx, const fsgpu_sharded_request* request, uint32_t* out_rows, float* out_scores,
                                  uint32_t* out_counts, uint32_t* out_fallbacks) {
    const fsgpu_status c = check_sharded_request(idx, request);
    if (c != FSGPU_OK) return c;
    if (request->nq && (!out_counts || (request->k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    // concurrent single-query callers share one search of the shards (same hits: the batched mode is exact, the two-pass
    // candidates are per query)
    if (idx->coalescer.enabled() && request->nq == 1 && request->k >= 1 && request->k <= 64 && !request->allow_bitmap && request->queries &&
        request->query_len == idx->impl.dimension() && idx->impl.record_count() > 0 &&
        (request->mode == FSGPU_SHARDED_EXACT || request->mode == FSGPU_SHARDED_INT8_TWO_PASS)) {
        if (out_fallbacks) *out_fallbacks = 0;
        const uint32_t mult = request->mode == FSGPU_SHARDED_INT8_TWO_PASS ? (request->candidate_multiplier ? request->candidate_multiplier : 1) : 0;
        return coalesced_sharded_search(idx, request->queries, request->query_len, request->k, mult, out_rows, out_scores, out_counts);
    }
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search(sharded_request(request), request->query_len, out_rows, out_scores, out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_sharded_set_coalescing(fsgpu_sharded* idx, uint32_t max_batch, uint32_t max_wait_us) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    idx->coalescer.configure(max_batch, max_wait_us);
    return FSGPU_OK;
}

fsgpu_status fsgpu_sharded_coalescing_stats(fsgpu_sharded* idx, uint64_t* batches, uint64_t* requests) {
    if (!idx || !batches || !requests) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    idx->coalescer.stats(batches, requests);
    return FSGPU_OK;
}

// queries resident in parts on several devices (data-parallel encoders): request->queries / queries_dev are ignored
fsgpu_status fsgpu_sharded_search_parts(fsgpu_sharded* idx, const fsgpu_sharded_request* request, const float* const* parts_dev,
                                        const uint32_t* part_counts, const int32_t* part_devices, uint32_t n_parts, uint32_t* out_rows,
                                        float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx || !request) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (request->mode < FSGPU_SHARDED_EXACT || request->mode > FSGPU_SHARDED_4BIT_TWO_PASS) return fail(FSGPU_ERR_INVALID_CONFIG, "unknown search mode");
    if (request->nq && (!n_parts || !parts_dev || !part_counts || !part_devices)) return fail(FSGPU_ERR_NULL_ARGUMENT, "query parts are required");
    if (request->nq && (!out_counts || (request->k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        fsgpu::ShardedIndex::Request r = sharded_request(request);
        r.queries = nullptr;
        r.queries_dev = nullptr;
        r.parts_dev = parts_dev;
        r.part_counts = part_counts;
        r.part_devices = part_devices;
        r.n_parts = n_parts;
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search(r, request->query_len, out_rows, out_scores, out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_sharded_search_begin(fsgpu_sharded* idx, const fsgpu_sharded_request* request, uint64_t* out_ticket) {
    const fsgpu_status c = check_sharded_request(idx, request);
    if (c != FSGPU_OK) return c;
    if (!out_ticket) return fail(FSGPU_ERR_NULL_ARGUMENT, "ticket is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.begin(sharded_request(request), request->query_len, out_ticket));
    });
}

fsgpu_status fsgpu_sharded_search_end(fsgpu_sharded* idx, uint64_t ticket, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                      uint32_t* out_fallbacks) {
    if (!idx || !out_counts) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.end(ticket, out_rows, out_scores, out_counts, out_fallbacks));
    });
}

static fsgpu_status sharded_search(fsgpu_sharded* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                   bool batched, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                   uint32_t* out_fallbacks) {
    fsgpu_sharded_request rq{queries, nq, query_len, k, batched ? FSGPU_SHARDED_BATCHED : FSGPU_SHARDED_EXACT, 0, nullptr, nullptr};
    return fsgpu_sharded_search(idx, &rq, out_rows, out_scores, out_counts, out_fallbacks);
}

fsgpu_status fsgpu_sharded_search_topk(fsgpu_sharded* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                       uint32_t* out_rows, float* out_scores, uint32_t* out_counts) {
    return sharded_search(idx, queries, nq, query_len, k, false, out_rows, out_scores, out_counts, nullptr);
}

fsgpu_status fsgpu_sharded_search_topk_batched(fsgpu_sharded* idx, const float* queries, uint32_t nq, uint32_t query_len,
                                               uint32_t k, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                               uint32_t* out_fallbacks) {
    return sharded_search(idx, queries, nq, query_len, k, true, out_rows, out_scores, out_counts, out_fallbacks);
}

float fsgpu_sharded_quant_scale_max(const fsgpu_sharded* idx) { return idx ? idx->impl.quant_scale_max() : 0.0f; }

fsgpu_status fsgpu_sharded_open_fsvi(const char* path, const int32_t* devices, uint32_t ndev, int32_t exchange, fsgpu_sharded** out) {
    return fsgpu_sharded_open_fsvi_grouped(path, devices, ndev, 1, exchange, out);
}

fsgpu_status fsgpu_sharded_open_fsvi_grouped(const char* path, const int32_t* devices, uint32_t ndev, uint32_t query_groups, int32_t exchange,
                                             fsgpu_sharded** out) {
    if (!out || !path || !devices) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_sharded();
        fsgpu::SearchError e = h->impl.open_fsvi(path, devices, ndev, exchange, query_groups);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_sharded_set_live_bitmap(fsgpu_sharded* idx, const uint64_t* live_bitmap) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.set_live_bitmap(live_bitmap));
    });
}

fsgpu_status fsgpu_sharded_soft_delete(fsgpu_sharded* idx, const char* doc_id, uint32_t doc_id_len, int32_t* out_deleted) {
    if (!idx || !out_deleted || (doc_id_len && !doc_id)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.soft_delete(doc_id, doc_id_len, out_deleted));
    });
}

fsgpu_status fsgpu_sharded_wal_append(fsgpu_sharded* idx, const char* doc_id, uint32_t doc_id_len, const float* vector,
                                      uint32_t vector_len) {
    if (!idx || !vector || (doc_id_len && !doc_id)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.wal_append(doc_id, doc_id_len, vector, vector_len));
    });
}

uint64_t fsgpu_sharded_wal_record_count(const fsgpu_sharded* idx) { return idx ? idx->impl.wal_record_count() : 0; }

fsgpu_status fsgpu_sharded_doc_id(const fsgpu_sharded* idx, uint32_t row, const char** out_ptr, uint32_t* out_len) {
    if (!idx || !out_ptr || !out_len) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return finish(idx->impl.doc_id_at(row, out_ptr, out_len));
}

fsgpu_status fsgpu_sharded_search_hits(fsgpu_sharded* idx, const float* query, uint32_t query_len, uint32_t k, uint32_t* out_rows,
                                       float* out_scores, uint32_t* out_count) {
    if (!idx || !query || !out_count || (k && (!out_rows || !out_scores))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_hits(query, query_len, k, out_rows, out_scores, out_count));
    });
}

fsgpu_status fsgpu_sharded_gather_dot(fsgpu_sharded* idx, const float* query, uint32_t query_len, const uint32_t* rows, uint32_t n,
                                      float* out_scores) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (n && (!query || !rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.gather_dot(query, query_len, rows, n, out_scores));
    });
}

fsgpu_status fsgpu_search_topk_classified(fsgpu_index* idx, const float* query, uint32_t query_len, uint32_t k,
                                          uint32_t* out_rows, float* out_scores, uint32_t* out_count,
                                          int32_t* zero_signal) {
    if (!idx || !query || !out_count || !zero_signal) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *zero_signal = FSGPU_ZERO_SIGNAL_NONE;
    *out_count = 0;
    if (query_len != idx->impl.dimension()) {
        g_last_error = "expected " + std::to_string(idx->impl.dimension()) + ", found " + std::to_string(query_len);
        return FSGPU_ERR_DIMENSION_MISMATCH;
    }
    if (k == 0) {
        *zero_signal = FSGPU_ZERO_SIGNAL_CALLER_REQUESTED_ZERO_K;
        return FSGPU_OK;
    }
    bool all_zero = true;
    for (uint32_t i = 0; i < query_len; ++i) {
        if (!std::isfinite(query[i])) return fail(FSGPU_ERR_INVALID_CONFIG, "query vector must be finite");
        if (query[i] != 0.0f) all_zero = false;
    }
    if (all_zero) {
        *zero_signal = FSGPU_ZERO_SIGNAL_ZERO_NORM_QUERY;
        return FSGPU_OK;
    }
    const bool table = idx->impl.has_doc_ids();
    fsgpu_status st = table ? fsgpu_search_hits(idx, query, query_len, k, out_rows, out_scores, out_count)
                            : fsgpu_search_topk(idx, query, 1, query_len, k, nullptr, out_rows, out_scores, out_count);
    if (st == FSGPU_OK && *out_count == 0) {
        // ZeroSignalState::empty_result_reason without a filter (config.rs:696-740).  The exact scan returns every live row
        // (a NaN score still ranks, search.rs:1655-1661), so an empty result means no live main record: the census the
        // reference computes lazily reduces to the record and WAL counts.
        // (the counts are read under the state lock a concurrent fsgpu_index_wal_append / soft_delete takes exclusively)
        uint64_t records, wal;
        {
            std::shared_lock<std::shared_mutex> state(idx->state_mu);
            records = idx->impl.record_count();
            wal = idx->impl.wal_record_count();
        }
        *zero_signal = records == 0 && wal == 0 ? FSGPU_ZERO_SIGNAL_NEWLY_CREATED_EMPTY
                       : wal == 0               ? FSGPU_ZERO_SIGNAL_ALL_TOMBSTONED
                                                : FSGPU_ZERO_SIGNAL_WAL_ONLY_NO_LIVE_RECORDS;
    }
    return st;
}

// search_top_k -> scan_wal -> resolve_sorted_entries (search.rs:426-494, 1449-1475, 1503-1558).
fsgpu_status fsgpu_search_hits(fsgpu_index* idx, const float* query, uint32_t query_len, uint32_t k,
                               uint32_t* out_rows, float* out_scores, uint32_t* out_count) {
    if (!idx || !query || !out_count) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_count = 0;
    if (k && (!out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_hits(query, query_len, k, out_rows, out_scores, out_count));
    });
}

// search_hits for a batch: WAL merge, shadowing and dedup on the device (vector_index_hits.cpp, search_hits_kernels.hip)
fsgpu_status fsgpu_search_hits_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                       uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_hits_batched(queries, nq, query_len, k, out_rows, out_scores, out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_search_hits_batched_device_queries(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                      uint32_t k, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                                      uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries_dev || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_hits_batched(queries_dev, nq, query_len, k, out_rows, out_scores, out_counts, out_fallbacks, true));
    });
}

fsgpu_status fsgpu_search_hits_two_pass_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                uint32_t candidate_multiplier, uint32_t bits, uint32_t* out_rows, float* out_scores,
                                                uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_hits_two_pass_batched(queries, nq, query_len, k, candidate_multiplier, (int)bits, out_rows, out_scores,
                                                             out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_lab_index_wal_scores(fsgpu_index* idx, const float* queries, uint32_t nq, float* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.lab_wal_scores(queries, nq, out));
    });
}

fsgpu_status fsgpu_search_topk_int8_two_pass_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t candidate_multiplier, uint32_t* out_rows,
                                                     float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_int8_batched(queries, nq, query_len, k, candidate_multiplier, out_rows,
                                                          out_scores, out_counts, out_fallbacks));
    });
}

fsgpu_status fsgpu_search_topk_4bit_two_pass_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t candidate_multiplier, uint32_t* out_rows,
                                                     float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores))))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_int8_batched(queries, nq, query_len, k, candidate_multiplier, out_rows,
                                                          out_scores, out_counts, out_fallbacks, 4));
    });
}

// VectorIndex::search_top_k_4bit_two_pass (search.rs:876-946)
fsgpu_status fsgpu_search_topk_4bit_two_pass(fsgpu_index* idx, const float* query, uint32_t query_len, uint32_t k,
                                             uint32_t candidate_multiplier, uint32_t* out_rows, float* out_scores,
                                             uint32_t* out_count) {
    if (!idx || !query || !out_count) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_count = 0;
    if (k && (!out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_4bit_two_pass(query, query_len, k, candidate_multiplier, out_rows,
                                                           out_scores, out_count));
    });
}

// VectorIndex::mrl_search_with_stats (mrl.rs:241-395)
fsgpu_status fsgpu_search_mrl(fsgpu_index* idx, const float* query, uint32_t query_len, uint32_t k, uint32_t search_dims,
                              uint32_t rescore_dims, uint32_t rescore_top_k, uint32_t* out_rows, float* out_scores,
                              uint32_t* out_count, fsgpu_mrl_stats* stats) {
    if (!idx || !query || !out_count) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_count = 0;
    if (k && (!out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        fsgpu::VectorIndex::MrlStats st;
        const fsgpu_status rc = finish(idx->impl.mrl_search(query, query_len, k, search_dims, rescore_dims, rescore_top_k,
                                                            out_rows, out_scores, out_count, &st));
        if (stats) {
            stats->scan_dims = st.scan_dims;
            stats->rescore_dims = st.rescore_dims;
            stats->candidates_rescored = st.candidates_rescored;
            stats->records_scanned = st.records_scanned;
            stats->fell_back_to_full = st.fell_back_to_full ? 1 : 0;
        }
        return rc;
    });
}

fsgpu_status fsgpu_search_mrl_batched(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                      uint32_t search_dims, uint32_t rescore_dims, uint32_t rescore_top_k, uint32_t* out_rows,
                                      float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.mrl_search_batched(queries, nq, query_len, k, search_dims, rescore_dims, rescore_top_k, out_rows,
                                                   out_scores, out_counts, out_fallbacks));
    });
}

// VectorIndex::search_top_k_int8_two_pass (search.rs:514-661)
fsgpu_status fsgpu_search_topk_int8_two_pass(fsgpu_index* idx, const float* query, uint32_t query_len, uint32_t k,
                                             uint32_t candidate_multiplier, uint32_t* out_rows, float* out_scores,
                                             uint32_t* out_count) {
    if (!idx || !query || !out_count) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_count = 0;
    if (k && (!out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (idx->coalescer.enabled() && k >= 1 && k <= 64 && query_len == idx->impl.dimension() && !idx->impl.has_doc_ids() &&
        idx->impl.wal_record_count() == 0)
        return coalesced_search(idx, query, k, candidate_multiplier ? candidate_multiplier : 1, out_rows, out_scores, out_count);
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_int8_two_pass(query, query_len, k, candidate_multiplier, out_rows,
                                                           out_scores, out_count));
    });
}

// VectorIndex::append (lib.rs:2532-2720)
fsgpu_status fsgpu_index_wal_append(fsgpu_index* idx, const char* doc_id, uint32_t doc_id_len, const float* vector,
                                    uint32_t vector_len) {
    if (!idx || !doc_id || !vector) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const fsgpu::SearchError e = idx->impl.wal_append(doc_id, doc_id_len, vector, vector_len);
        idx->impl.sync_replicas();   // the shadowed main row was tombstoned
        return finish(e);
    });
}

uint64_t fsgpu_index_wal_record_count(const fsgpu_index* idx) { return idx ? idx->impl.wal_record_count() : 0; }

// VectorIndex::append_batch (lib.rs:2546-2720)
fsgpu_status fsgpu_index_wal_append_batch(fsgpu_index* idx, uint32_t n, const char* const* doc_ids, const uint32_t* doc_id_lens,
                                          const float* vectors, uint32_t vector_len) {
    if (!idx || (n && (!doc_ids || !doc_id_lens || !vectors))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const fsgpu::SearchError e = idx->impl.wal_append_batch(n, doc_ids, doc_id_lens, vectors, vector_len);
        idx->impl.sync_replicas();   // the shadowed main rows were tombstoned
        return finish(e);
    });
}

// VectorIndex::compact (lib.rs:2734-2854)
fsgpu_status fsgpu_index_compact(fsgpu_index* idx, const char* path, fsgpu_compaction_stats* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return rewrite_locked(idx, [&]() {
        fsgpu::VectorIndex::CompactionStats st;
        const fsgpu::SearchError e = idx->impl.compact(path, &st);
        if (e.ok() && out) *out = fsgpu_compaction_stats{st.main_records_before, st.wal_records, st.total_records_after, st.elapsed_ms};
        return e;
    });
}

// VectorIndex::vacuum (lib.rs:2485-2521)
fsgpu_status fsgpu_index_vacuum(fsgpu_index* idx, const char* path, fsgpu_vacuum_stats* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return rewrite_locked(idx, [&]() {
        fsgpu::VectorIndex::VacuumStats st;
        const fsgpu::SearchError e = idx->impl.vacuum(path, &st);
        if (e.ok() && out) *out = fsgpu_vacuum_stats{st.records_before, st.records_after, st.tombstones_removed, st.bytes_reclaimed, st.elapsed_ms};
        return e;
    });
}

// VectorIndex::needs_compaction (lib.rs:2270-2292)
fsgpu_status fsgpu_index_needs_compaction(fsgpu_index* idx, uint64_t threshold, double ratio, int32_t* out) {
    if (!idx || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    *out = idx->impl.needs_compaction(threshold, ratio) ? 1 : 0;
    return FSGPU_OK;
}

// VectorIndex::needs_vacuum (lib.rs:174, 2464-2475)
fsgpu_status fsgpu_index_needs_vacuum(fsgpu_index* idx, int32_t* out) {
    if (!idx || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const fsgpu::SearchError e = idx->impl.fetch_live_host();
        if (!e.ok()) return finish(e);
        *out = idx->impl.needs_vacuum() ? 1 : 0;
        return FSGPU_OK;
    });
}

static uint64_t counted_rows(fsgpu_index* idx, bool tombstones) {
    if (!idx) return 0;
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    if (!idx->impl.fetch_live_host().ok()) return 0;
    return tombstones ? idx->impl.tombstone_count() : idx->impl.live_count();
}
uint64_t fsgpu_index_tombstone_count(fsgpu_index* idx) { return counted_rows(idx, true); }   /* VectorIndex::tombstone_count */
uint64_t fsgpu_index_live_count(fsgpu_index* idx) { return counted_rows(idx, false); }

uint64_t fsgpu_index_generation(const fsgpu_index* idx) { return idx ? idx->impl.generation() : 0; }
uint32_t fsgpu_index_compaction_gen(const fsgpu_index* idx) { return idx ? idx->impl.compaction_gen() : 0; }

// a row-sharded handle refuses both: the rows would have to be re-sharded and exchanged
fsgpu_status fsgpu_sharded_compact(fsgpu_sharded* idx, const char* path, fsgpu_compaction_stats* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    (void)out;
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.compact(path));
    });
}
fsgpu_status fsgpu_sharded_vacuum(fsgpu_sharded* idx, const char* path, fsgpu_vacuum_stats* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    (void)out;
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.vacuum(path));
    });
}

// ---- lab (include/fsgpu_lab.h) ----
fsgpu_status fsgpu_lab_index_set_compact_launch_rows(fsgpu_index* idx, uint32_t rows) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.compact_launch_rows = rows;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_set_compact_nt_stores(fsgpu_index* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.compact_nt_stores = enabled != 0;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_last_rewrite(fsgpu_index* idx, double* out_ms5, uint64_t* out_counts3) {
    if (!idx || !out_ms5 || !out_counts3) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    const fsgpu::VectorIndex::RewriteTimes& t = idx->impl.last_rewrite;
    out_ms5[0] = t.plan_ms, out_ms5[1] = t.kernel_ms, out_ms5[2] = t.tables_ms, out_ms5[3] = t.file_ms, out_ms5[4] = t.rebuild_ms;
    out_counts3[0] = t.runs, out_counts3[1] = t.launches, out_counts3[2] = t.dst_bytes;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_attach_synthetic_doc_ids(fsgpu_index* idx) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.lab_attach_synthetic_doc_ids());
    });
}
fsgpu_status fsgpu_lab_device_copy_ms(int32_t device, uint64_t bytes, uint32_t reps, double* out_ms) {
    if (!out_ms && reps) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_NO_DEVICE, "hipSetDevice failed");
        fsgpu::DeviceBuffer a, b;
        fsgpu::SearchError e = a.reserve((size_t)bytes);
        if (e.ok()) e = b.reserve((size_t)bytes);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t he = hipSuccess;
        if (e.ok()) he = hipMemset(a.ptr, 1, (size_t)bytes);
        if (e.ok() && he == hipSuccess) he = hipEventCreate(&e0);
        if (e.ok() && he == hipSuccess) he = hipEventCreate(&e1);
        for (uint32_t r = 0; e.ok() && he == hipSuccess && r < reps; ++r) {
            he = hipEventRecord(e0, nullptr);
            if (he == hipSuccess) he = hipMemcpyAsync(b.ptr, a.ptr, (size_t)bytes, hipMemcpyDeviceToDevice, nullptr);
            if (he == hipSuccess) he = hipEventRecord(e1, nullptr);
            if (he == hipSuccess) he = hipEventSynchronize(e1);
            float ms = 0.f;
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
            out_ms[r] = ms;
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        a.release();
        b.release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_gather_dot(fsgpu_index* idx, const float* query, uint32_t query_len, const uint32_t* rows,
                              uint32_t n, float* out_scores) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (n && (!query || !rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.gather_dot(query, query_len, rows, n, out_scores));
    });
}

fsgpu_status fsgpu_alignment_create(fsgpu_index* fast, fsgpu_index* quality, fsgpu_alignment** out) {
    if (!fast || !quality || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto a = std::make_unique<fsgpu_alignment>();
        std::shared_lock<std::shared_mutex> lf(fast->state_mu);
        std::shared_lock<std::shared_mutex> lq(quality->state_mu, std::defer_lock);
        if (quality != fast) lq.lock();
        const fsgpu_status st = finish(a->impl.build(fast->impl, quality->impl));
        if (st == FSGPU_OK) *out = a.release();
        return st;
    });
}

void fsgpu_alignment_destroy(fsgpu_alignment* a) { delete a; }
int32_t fsgpu_alignment_kind(const fsgpu_alignment* a) { return a ? (int32_t)a->impl.kind() : FSGPU_ALIGNMENT_NONE; }
int64_t fsgpu_alignment_quality_row(const fsgpu_alignment* a, uint64_t fast_row) { return a ? a->impl.quality_row(fast_row) : -1; }
uint64_t fsgpu_alignment_unmatched_quality_docs(const fsgpu_alignment* a) { return a ? a->impl.unmatched_quality_docs() : 0; }

fsgpu_status fsgpu_quality_scores_for_hits(fsgpu_index* fast, fsgpu_index* quality, const fsgpu_alignment* alignment,
                                           const float* query, uint32_t query_len, const fsgpu_scored_doc* hits, uint32_t n,
                                           float* out_scores, uint8_t* out_present) {
    if (!fast || !quality || !alignment) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (n && (!query || !hits || !out_scores || !out_present)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::HitRef> refs(n);
        for (uint32_t i = 0; i < n; ++i) refs[i] = fsgpu::HitRef{hits[i].doc_id, hits[i].doc_id_len, hits[i].index};
        std::shared_lock<std::shared_mutex> lf(fast->state_mu);
        std::shared_lock<std::shared_mutex> lq(quality->state_mu, std::defer_lock);
        if (quality != fast) lq.lock();
        return finish(fsgpu::quality_scores_for_hits(fast->impl, quality->impl, alignment->impl, query, query_len, refs.data(), n,
                                                     out_scores, out_present));
    });
}

fsgpu_status fsgpu_quality_scores_for_hits_batched(fsgpu_index* fast, fsgpu_index* quality, const fsgpu_alignment* alignment,
                                                   const float* queries, uint32_t nq, uint32_t query_len, const fsgpu_scored_doc* hits,
                                                   const uint32_t* hit_offsets, float* out_scores, uint8_t* out_present) {
    if (!fast || !quality || !alignment) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (nq && (!queries || !hit_offsets)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const uint32_t n = nq ? hit_offsets[nq] : 0;
    if (n && (!hits || !out_scores || !out_present)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::HitRef> refs(n);
        for (uint32_t i = 0; i < n; ++i) refs[i] = fsgpu::HitRef{hits[i].doc_id, hits[i].doc_id_len, hits[i].index};
        std::shared_lock<std::shared_mutex> lf(fast->state_mu);
        std::shared_lock<std::shared_mutex> lq(quality->state_mu, std::defer_lock);
        if (quality != fast) lq.lock();
        return finish(fsgpu::quality_scores_for_hits_batched(fast->impl, quality->impl, alignment->impl, queries, nq, query_len, refs.data(),
                                                             hit_offsets, out_scores, out_present));
    });
}

// fsgpu_mmr_config: NULL = the reference's defaults (disabled, lambda 0.7, pool 30); enabled 0 / 1 and zero reserved words
fsgpu_status mmr_config_of(const fsgpu_mmr_config* config, fsgpu_mmr_config* out) {
    fsgpu_mmr_config_default(out);
    if (!config) return FSGPU_OK;
    for (uint32_t r : config->reserved)
        if (r != 0) return fail(FSGPU_ERR_INVALID_CONFIG, "fsgpu_mmr_config: reserved words must be 0");
    if (config->enabled > 1) return fail(FSGPU_ERR_INVALID_CONFIG, "fsgpu_mmr_config: enabled must be 0 or 1");
    *out = *config;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_vector_at_f32(fsgpu_index* idx, uint32_t row, float* out) {
    if (!idx || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.vector_at_f32(row, out));
    });
}

fsgpu_status fsgpu_index_mmr_rerank_batched(fsgpu_index* idx, const uint32_t* rows, const double* scores, const uint32_t* offsets, uint32_t nq,
                                            uint32_t k, const fsgpu_mmr_config* config, uint32_t* out_order, uint32_t* out_counts) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    fsgpu_mmr_config cfg;
    if (fsgpu_status st = mmr_config_of(config, &cfg)) return st;
    if (nq && (!offsets || !out_counts)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (nq && offsets[nq] && (!rows || !scores || !out_order)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.mmr_rerank_rows(rows, scores, offsets, nq, k, cfg.lambda, cfg.candidate_pool, nullptr, nullptr, 0, out_order,
                                                out_counts, nullptr));
    });
}

fsgpu_status fsgpu_index_mmr_rerank(fsgpu_index* idx, const uint32_t* rows, const double* scores, uint32_t n, uint32_t k,
                                    const fsgpu_mmr_config* config, uint32_t* out_order, uint32_t* out_count, double* out_sims) {
    if (!idx || !out_count) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_count = 0;
    fsgpu_mmr_config cfg;
    if (fsgpu_status st = mmr_config_of(config, &cfg)) return st;
    if (n && (!rows || !scores || !out_order)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const uint32_t offsets[2] = {0, n};
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.mmr_rerank_rows(rows, scores, offsets, 1, k, cfg.lambda, cfg.candidate_pool, nullptr, nullptr, 0, out_order,
                                                out_count, out_sims));
    });
}

fsgpu_status fsgpu_index_mmr_rerank_docs(fsgpu_index* idx, const fsgpu_scored_doc* docs, uint32_t n, const fsgpu_mmr_config* config,
                                         uint32_t* out_order, uint8_t* out_applied) {
    if (!idx || !out_applied) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_applied = 0;
    fsgpu_mmr_config cfg;
    if (fsgpu_status st = mmr_config_of(config, &cfg)) return st;
    if (n && (!docs || !out_order)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<const char*> ids(n);
        std::vector<uint32_t> lens(n);
        std::vector<float> scores(n);
        for (uint32_t i = 0; i < n; ++i) {
            if (!docs[i].doc_id && docs[i].doc_id_len) return fail(FSGPU_ERR_NULL_ARGUMENT, "doc id is null");
            ids[i] = docs[i].doc_id ? docs[i].doc_id : "";
            lens[i] = docs[i].doc_id_len;
            scores[i] = docs[i].score;
        }
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.mmr_rerank_docs(ids.data(), lens.data(), scores.data(), n, cfg.enabled != 0, cfg.lambda, cfg.candidate_pool,
                                                out_order, out_applied));
    });
}

fsgpu_status fsgpu_two_tier_mmr_rerank(fsgpu_index* fast, fsgpu_index* quality, const fsgpu_alignment* alignment, const fsgpu_scored_doc* hits,
                                       uint32_t n, const fsgpu_mmr_config* config, uint32_t* out_order, uint8_t* out_applied) {
    if (!fast || !quality || !alignment || !out_applied) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out_applied = 0;
    fsgpu_mmr_config cfg;
    if (fsgpu_status st = mmr_config_of(config, &cfg)) return st;
    if (n && (!hits || !out_order)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::HitRef> refs(n);
        std::vector<float> scores(n);
        for (uint32_t i = 0; i < n; ++i) {
            refs[i] = fsgpu::HitRef{hits[i].doc_id, hits[i].doc_id_len, hits[i].index};
            scores[i] = hits[i].score;
        }
        std::shared_lock<std::shared_mutex> lf(fast->state_mu);
        std::shared_lock<std::shared_mutex> lq(quality->state_mu, std::defer_lock);
        if (quality != fast) lq.lock();
        return finish(fsgpu::two_tier_mmr_rerank(fast->impl, quality->impl, alignment->impl, refs.data(), scores.data(), n, cfg.enabled != 0,
                                                 cfg.lambda, cfg.candidate_pool, out_order, out_applied));
    });
}

static fsgpu_status index_query_hubness(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq, float* out,
                                        float* out_topk) {
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (idx->impl.record_count() && !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    if (nq && !queries) return fail(FSGPU_ERR_NULL_ARGUMENT, "queries is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.compute_query_hubness(queries, nq, query_dim, kq, out, out_topk));
    });
}

fsgpu_status fsgpu_index_compute_query_hubness(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                               float* out) {
    return index_query_hubness(idx, queries, nq, query_dim, kq, out, nullptr);
}

fsgpu_status fsgpu_lab_index_query_hubness_topk(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                                float* out, float* out_topk) {
    if (idx && idx->impl.record_count() && !out_topk) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_topk is null");
    return index_query_hubness(idx, queries, nq, query_dim, kq, out, out_topk);
}

fsgpu_status fsgpu_sharded_compute_query_hubness(fsgpu_sharded* sh, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                                 float* out) {
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!sh) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (sh->impl.record_count() && !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    if (nq && !queries) return fail(FSGPU_ERR_NULL_ARGUMENT, "queries is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(sh->impl.mutex());
        return finish(sh->impl.compute_query_hubness(queries, nq, query_dim, kq, out));
    });
}

// the k-NN graph: errors are reported before any work starts — m, then the device, then the handle and its range
fsgpu_status fsgpu_index_build_knn_graph(fsgpu_index* idx, uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t* out_rows,
                                         float* out_sims) {
    if (m < 1 || m > fsgpu::kKnnMaxM) return fail(FSGPU_ERR_INVALID_CONFIG, "m must be 1 .. 63 (k = m + 1 stays inside the fused tiers)");
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        const uint64_t n = idx->impl.record_count();
        if (first_row > n || n_rows > n - first_row) return fail(FSGPU_ERR_INVALID_CONFIG, "the source rows lie past record_count");
        if (n_rows && !out_rows) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_rows is null");
        return finish(idx->impl.build_knn_graph(first_row, n_rows, m, out_rows, out_sims));
    });
}

// the graph optimisation: the shape is judged first, then the device, then the handle and its row count; nothing is written on a refusal
fsgpu_status fsgpu_knn_graph_optimize(fsgpu_index* idx, const uint32_t* graph_rows, uint64_t graph_len, uint32_t graph_width,
                                      uint32_t out_degree, uint32_t* out_rows, fsgpu_knn_optimize_stats* stats) {
    if (graph_width > fsgpu::kKnnOptMaxWidth) return fail(FSGPU_ERR_INVALID_CONFIG, "graph_width must be at most 64 (a list is one wave wide)");
    if (out_degree < 1 || out_degree > graph_width) return fail(FSGPU_ERR_INVALID_CONFIG, "out_degree must be 1 .. graph_width");
    if (graph_len && (!graph_rows || !out_rows)) return fail(FSGPU_ERR_INVALID_CONFIG, "the table and the output must not be null");
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        if (graph_len != idx->impl.record_count())
            return fail(FSGPU_ERR_INVALID_CONFIG, ("graph_len " + std::to_string(graph_len) + " is not record_count " +
                                                   std::to_string(idx->impl.record_count())).c_str());
        fsgpu::VectorIndex::KnnOptimizeStats st;
        const fsgpu_status s = finish(idx->impl.optimize_knn_graph(graph_rows, graph_width, out_degree, out_rows, stats ? &st : nullptr));
        if (s == FSGPU_OK && stats) {
            std::memset(stats, 0, sizeof(*stats));
            stats->rows = st.rows;
            stats->forward_edges = st.forward_edges;
            stats->reverse_edges = st.reverse_edges;
            stats->zero_in_degree_before = st.zero_in_degree_before;
            stats->zero_in_degree_after = st.zero_in_degree_after;
            stats->max_detour_count = st.max_detour_count;
            stats->device_ms = st.device_ms;
        }
        return s;
    });
}

fsgpu_status fsgpu_lab_index_knn_build_stats(fsgpu_index* idx, uint64_t* out4) {
    if (!idx || !out4) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    const fsgpu::VectorIndex::KnnBuildStats& st = idx->impl.last_knn_build;
    out4[0] = st.steps, out4[1] = st.sources, out4[2] = st.fallbacks, out4[3] = st.late_answers;
    return FSGPU_OK;
}

fsgpu_status fsgpu_sharded_build_knn_graph(fsgpu_sharded* sh, uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t* out_rows,
                                           float* out_sims) {
    if (m < 1 || m > fsgpu::kKnnMaxM) return fail(FSGPU_ERR_INVALID_CONFIG, "m must be 1 .. 63 (k = m + 1 stays inside the fused tiers)");
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!sh) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(sh->impl.mutex());
        const uint64_t n = sh->impl.record_count();
        if (first_row > n || n_rows > n - first_row) return fail(FSGPU_ERR_INVALID_CONFIG, "the source rows lie past record_count");
        if (n_rows && !out_rows) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_rows is null");
        return finish(sh->impl.build_knn_graph(first_row, n_rows, m, out_rows, out_sims));
    });
}

// ---- graph ANN search over the k-NN table (ann_index.cpp, ann_kernels.hip; hnsw.rs:842-1330, 1354-1386) ----
fsgpu_status fsgpu_ann_config_default(fsgpu_ann_config* config) {
    if (!config) return fail(FSGPU_ERR_NULL_ARGUMENT, "config is null");
    const fsgpu::AnnConfig d;
    std::memset(config, 0, sizeof(*config));
    config->n_entry = d.n_entry;
    config->degree = d.degree;
    config->expand = d.expand;
    config->max_iters = d.max_iters;
    return FSGPU_OK;
}

fsgpu_status fsgpu_ann_create(fsgpu_index* idx, const uint32_t* graph_rows, uint64_t graph_len, uint32_t graph_width,
                              const fsgpu_ann_config* config, fsgpu_ann** out) {
    if (!idx || !out || (!graph_rows && graph_len)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    fsgpu::AnnConfig c;
    if (config) {
        for (uint32_t r : config->reserved)
            if (r) return fail(FSGPU_ERR_INVALID_CONFIG, "reserved words of fsgpu_ann_config must be 0");
        c.n_entry = config->n_entry;
        c.degree = config->degree;
        c.expand = config->expand;
        c.max_iters = config->max_iters;
    }
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        auto a = std::make_unique<fsgpu_ann>();
        a->idx = idx;
        const fsgpu::SearchError e = a->impl.init(&idx->impl, graph_rows, graph_len, graph_width, c);
        if (!e.ok()) return finish(e);
        *out = a.release();
        return FSGPU_OK;
    });
}

void fsgpu_ann_destroy(fsgpu_ann* ann) { delete ann; }
uint64_t fsgpu_ann_record_count(const fsgpu_ann* ann) { return ann ? ann->impl.record_count() : 0; }
int32_t fsgpu_ann_device(const fsgpu_ann* ann) { return ann ? ann->impl.device() : -1; }

static fsgpu_status ann_search_common(fsgpu_ann* ann, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t ef,
                                      uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* out_flags, bool on_device,
                                      fsgpu_ann_stats* stats) {
    if (!ann) return fail(FSGPU_ERR_NULL_ARGUMENT, "handle is null");
    if (nq && (!queries || !out_counts || !out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ann->idx->state_mu);
        std::lock_guard<std::mutex> lock(ann->idx->impl.mutex());
        fsgpu::AnnStats st;
        const fsgpu::SearchError e = ann->impl.search(queries, nq, query_len, k, ef, out_rows, out_scores, out_counts, out_flags, on_device, &st);
        if (e.ok() && stats) ann_stats_out(st, stats);
        return finish(e);
    });
}

fsgpu_status fsgpu_ann_search_batched(fsgpu_ann* ann, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t ef,
                                      uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* out_flags,
                                      fsgpu_ann_stats* stats) {
    return ann_search_common(ann, queries, nq, query_len, k, ef, out_rows, out_scores, out_counts, out_flags, false, stats);
}

fsgpu_status fsgpu_ann_search_batched_device_queries(fsgpu_ann* ann, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t ef, uint32_t* out_rows_dev, float* out_scores_dev,
                                                     uint32_t* out_counts_dev, uint32_t* out_flags_dev, fsgpu_ann_stats* stats) {
    return ann_search_common(ann, queries_dev, nq, query_len, k, ef, out_rows_dev, out_scores_dev, out_counts_dev, out_flags_dev, true, stats);
}

fsgpu_status fsgpu_ann_search(fsgpu_ann* ann, const float* query, uint32_t query_len, uint32_t k, uint32_t ef, uint32_t* out_rows,
                              float* out_scores, uint32_t* out_count, uint32_t* out_flag, fsgpu_ann_stats* stats) {
    return ann_search_common(ann, query, 1, query_len, k, ef, out_rows, out_scores, out_count, out_flag, false, stats);
}

fsgpu_status fsgpu_ann_last_stats(const fsgpu_ann* ann, fsgpu_ann_stats* stats) {
    if (!ann || !stats) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(ann->idx->impl.mutex());
    ann_stats_out(ann->impl.last_stats(), stats);
    return FSGPU_OK;
}

fsgpu_status fsgpu_ann_certify_ef(fsgpu_ann* ann, const float* queries, uint32_t nq, const uint32_t* candidate_efs, uint32_t n_efs,
                                  uint32_t k, double target, double alpha, fsgpu_certified_ef* chosen, fsgpu_certified_ef* sweep_out,
                                  uint32_t* n_swept) {
    if (!ann || !chosen || !sweep_out || !n_swept || (!queries && nq) || (!candidate_efs && n_efs))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ann->idx->state_mu);
        std::lock_guard<std::mutex> lock(ann->idx->impl.mutex());
        std::vector<fsgpu::CertifiedEf> sweep(n_efs);
        fsgpu::CertifiedEf best;
        uint32_t swept = 0;
        const fsgpu::SearchError e = ann->impl.certify_ef(queries, nq, candidate_efs, n_efs, k, target, alpha, &best, sweep.data(), &swept);
        if (!e.ok()) return finish(e);
        for (uint32_t i = 0; i < swept; ++i) certified_out(sweep[i], &sweep_out[i]);
        certified_out(best, chosen);
        *n_swept = swept;
        return FSGPU_OK;
    });
}

double fsgpu_conformal_recall_lower_bound(const double* recalls, uint64_t n, double alpha) {
    return (recalls || !n) ? fsgpu::conformal_recall_lower_bound(recalls, n, alpha) : 0.0;
}
double fsgpu_mean_recall_lower_bound(const double* recalls, uint64_t n, double delta) {
    return (recalls || !n) ? fsgpu::mean_recall_lower_bound(recalls, n, delta) : 0.0;
}
double fsgpu_mean_recall_lower_bound_bernstein(const double* recalls, uint64_t n, double delta) {
    return (recalls || !n) ? fsgpu::mean_recall_lower_bound_bernstein(recalls, n, delta) : 0.0;
}

static fsgpu_status certified_min_ef_common(const uint32_t* efs, const double* const* recalls, const uint64_t* lens, uint32_t n, double target,
                                            double level, bool mean_bound, fsgpu_certified_ef* out) {
    if (!out || (n && (!efs || !recalls || !lens))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    for (uint32_t i = 0; i < n; ++i)
        if (!recalls[i] && lens[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "a recall sample is null");
    return guarded([&]() -> fsgpu_status {
        fsgpu::CertifiedEf c;
        if (!fsgpu::certified_min_ef(efs, recalls, lens, n, target, level, mean_bound, &c))
            return fail(FSGPU_ERR_INVALID_CONFIG, "the calibration is empty");
        certified_out(c, out);
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_certified_min_ef(const uint32_t* efs, const double* const* recalls, const uint64_t* lens, uint32_t n, double target,
                                    double alpha, fsgpu_certified_ef* out) {
    return certified_min_ef_common(efs, recalls, lens, n, target, alpha, false, out);
}

fsgpu_status fsgpu_certified_min_ef_mean(const uint32_t* efs, const double* const* recalls, const uint64_t* lens, uint32_t n,
                                         double target, double delta, fsgpu_certified_ef* out) {
    return certified_min_ef_common(efs, recalls, lens, n, target, delta, true, out);
}

// The same pairing over two row-sharded handles: the walk runs over their catalogs (fsgpu_sharded_open_fsvi) — raw shards pair by
// row —, the re-scoring gathers dot_query_at on the shards that own the quality rows (fsgpu_sharded_gather_dot).
fsgpu_status fsgpu_sharded_alignment_create(fsgpu_sharded* fast, fsgpu_sharded* quality, fsgpu_alignment** out) {
    if (!fast || !quality || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto a = std::make_unique<fsgpu_alignment>();
        std::unique_lock<std::mutex> lf(fast->impl.mutex());
        std::unique_lock<std::mutex> lq(quality->impl.mutex(), std::defer_lock);
        if (quality != fast) lq.lock();
        const fsgpu_status st = finish(a->impl.build(fast->impl.catalog(), fast->impl.record_count(), quality->impl.catalog(),
                                                     quality->impl.record_count()));
        if (st == FSGPU_OK) *out = a.release();
        return st;
    });
}

fsgpu_status fsgpu_sharded_quality_scores_for_hits(fsgpu_sharded* fast, fsgpu_sharded* quality, const fsgpu_alignment* alignment,
                                                   const float* query, uint32_t query_len, const fsgpu_scored_doc* hits, uint32_t n,
                                                   float* out_scores, uint8_t* out_present) {
    if (!fast || !quality || !alignment) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (n && (!query || !hits || !out_scores || !out_present)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::vector<fsgpu::HitRef> refs(n);
        for (uint32_t i = 0; i < n; ++i) refs[i] = fsgpu::HitRef{hits[i].doc_id, hits[i].doc_id_len, hits[i].index};
        // The fast side is read through its record table AND its tombstones (find_index_by_doc_id), which fsgpu_sharded_soft_delete /
        // _wal_append change under fast's mutex; the quality handle is held for the gather.  Fast first, then quality: the order of
        // fsgpu_sharded_alignment_create.
        std::unique_lock<std::mutex> lf(fast->impl.mutex());
        std::unique_lock<std::mutex> lq(quality->impl.mutex(), std::defer_lock);
        if (quality != fast) lq.lock();
        fsgpu::QualityTierView view;
        view.table = quality->impl.catalog();
        view.rows = quality->impl.record_count();
        view.dim = quality->impl.dimension();
        view.gather = [quality](const float* q, uint32_t len, const uint32_t* rows, uint32_t cnt, float* out) {
            return quality->impl.gather_dot(q, len, rows, cnt, out);
        };
        return finish(fsgpu::quality_scores_for_hits(fast->impl.catalog(), fast->impl.record_count(), view, alignment->impl, query,
                                                     query_len, refs.data(), n, out_scores, out_present));
    });
}

static fsgpu_status convert_on_device(int32_t device, const void* src, size_t src_elem, uint64_t n, void* dst,
                                      size_t dst_elem, bool encode) {
    if (n == 0) return FSGPU_OK;
    if (!src || !dst) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
    return guarded([&]() -> fsgpu_status {
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        fsgpu::DeviceBuffer a, b;
        fsgpu::SearchError e = a.reserve((size_t)n * src_elem);
        if (e.ok()) e = b.reserve((size_t)n * dst_elem);
        if (!e.ok()) {
            a.release();
            b.release();
            return finish(e);
        }
        hipError_t he = hipMemcpy(a.ptr, src, (size_t)n * src_elem, hipMemcpyHostToDevice);
        if (he == hipSuccess)
            he = encode ? fsgpu::launch_encode_f16(static_cast<const float*>(a.ptr), (size_t)n,
                                                   static_cast<unsigned short*>(b.ptr), nullptr)
                        : fsgpu::launch_widen_f16(static_cast<const unsigned short*>(a.ptr), (size_t)n,
                                                  static_cast<float*>(b.ptr), nullptr);
        if (he == hipSuccess) he = hipMemcpy(dst, b.ptr, (size_t)n * dst_elem, hipMemcpyDeviceToHost);
        a.release();
        b.release();
        if (he != hipSuccess) {
            g_last_error = hipGetErrorString(he);
            return FSGPU_ERR_DEVICE;
        }
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_fsvi_write(const char* path, const char* embedder_id, const char* embedder_revision, uint32_t dim,
                              uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors,
                              uint8_t compaction_gen, int32_t device) {
    if (n >= 0x7fffffffull) return fail(FSGPU_ERR_INVALID_CONFIG, "record count must fit the launch grid");
    return guarded([&]() -> fsgpu_status {
        return finish(fsgpu::write_fsvi_v1(path, embedder_id, embedder_revision, dim, n, doc_ids, doc_id_lens, vectors,
                                           compaction_gen, device));
    });
}

fsgpu_status fsgpu_fsvi_write_quant(const char* path, const char* embedder_id, const char* embedder_revision, uint32_t dim,
                                    uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens,
                                    const float* vectors, uint8_t compaction_gen, int32_t device, uint8_t quantization) {
    if (n >= 0x7fffffffull) return fail(FSGPU_ERR_INVALID_CONFIG, "record count must fit the launch grid");
    return guarded([&]() -> fsgpu_status {
        return finish(fsgpu::write_fsvi_v1(path, embedder_id, embedder_revision, dim, n, doc_ids, doc_id_lens, vectors,
                                           compaction_gen, device, quantization));
    });
}

fsgpu_status fsgpu_bench_fixture_device(int32_t device, uint64_t first, uint64_t n, uint32_t dim, uint32_t clusters, float noise,
                                        uint64_t seed_base, int32_t as_f16, void* out_dev, void* hip_stream) {
    if (n && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_dev is null");
    if (dim == 0 || clusters == 0) return fail(FSGPU_ERR_INVALID_CONFIG, "dim and clusters must be positive");
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        fsgpu::DeviceBuffer cent;
        fsgpu::SearchError e = cent.reserve((size_t)clusters * dim * 4);
        if (!e.ok()) return finish(e);
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        hipError_t he = fsgpu::launch_bench_fixture(first, n, dim, clusters, noise, seed_base, static_cast<float*>(cent.ptr),
                                                    as_f16 ? static_cast<unsigned short*>(out_dev) : nullptr,
                                                    as_f16 ? nullptr : static_cast<float*>(out_dev), st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        cent.release();
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_sort_keys_desc(int32_t device, const uint64_t* keys, uint64_t n, uint64_t varying_bits, uint64_t* out_sorted) {
    if (n && (!keys || !out_sorted)) return fail(FSGPU_ERR_NULL_ARGUMENT, "keys / out_sorted is null");
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        if (n == 0) return FSGPU_OK;
        fsgpu::DeviceBuffer in, out, tmp;
        size_t tmp_bytes = 0;
        (void)fsgpu::sort_keys_desc_temp_bytes(n, &tmp_bytes);
        fsgpu::SearchError e = in.reserve(n * 8);
        if (e.ok()) e = out.reserve(n * 8);
        if (e.ok()) e = tmp.reserve(tmp_bytes);
        hipError_t he = hipSuccess;
        if (e.ok()) {
            he = hipMemcpy(in.ptr, keys, n * 8, hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = fsgpu::sort_keys_desc(tmp.ptr, tmp.bytes, static_cast<const fsgpu::u64*>(in.ptr), static_cast<fsgpu::u64*>(out.ptr), n, nullptr, varying_bits);
            if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
            if (he == hipSuccess) he = hipMemcpy(out_sorted, out.ptr, n * 8, hipMemcpyDeviceToHost);
        }
        in.release();
        out.release();
        tmp.release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_encode_f32_to_f16(int32_t device, const float* src, uint64_t n, uint16_t* dst) {
    return convert_on_device(device, src, 4, n, dst, 2, true);
}

fsgpu_status fsgpu_widen_f16_to_f32(int32_t device, const uint16_t* src, uint64_t n, float* dst) {
    return convert_on_device(device, src, 2, n, dst, 4, false);
}

fsgpu_status fsgpu_m2v_create(int32_t device, const float* table, uint32_t vocab, uint32_t dim, fsgpu_m2v** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_m2v();
        fsgpu::SearchError e = h->impl.init(device, table, vocab, dim);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

void fsgpu_m2v_destroy(fsgpu_m2v* m) { delete m; }

fsgpu_status fsgpu_m2v_embed_device(fsgpu_m2v* m, const uint32_t* ids, const uint32_t* offsets, uint32_t n, float* out_dev) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (n && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_dev is null");
    return guarded([&]() -> fsgpu_status { return finish(m->impl.embed_batch(ids, offsets, n, nullptr, out_dev)); });
}
uint32_t fsgpu_m2v_dimension(const fsgpu_m2v* m) { return m ? m->impl.dimension() : 0; }

fsgpu_status fsgpu_m2v_embed(fsgpu_m2v* m, const uint32_t* ids, const uint32_t* offsets, uint32_t n, float* out) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (m->coalescer.enabled() && n == 1 && offsets && out && (ids || offsets[1] == offsets[0])) {
        return guarded([&]() -> fsgpu_status {
            EmbedCall<uint32_t> call;
            call.ids = ids ? ids + offsets[0] : nullptr;
            call.len = offsets[1] - offsets[0];
            call.out = out;
            m->coalescer.submit(
                &call, [m](std::vector<EmbedCall<uint32_t>*>& batch) { run_embed_batch(m, m->impl.dimension(), batch); },
                [](const EmbedCall<uint32_t>&, const EmbedCall<uint32_t>&) { return true; });
            if (call.exec_threw) return fail(FSGPU_ERR_DEVICE, "coalesced batch failed before this request was served");
            if (call.status != FSGPU_OK) g_last_error = call.detail;
            return call.status;
        });
    }
    return guarded([&]() -> fsgpu_status { return finish(m->impl.embed_batch(ids, offsets, n, out)); });
}

fsgpu_status fsgpu_m2v_set_coalescing(fsgpu_m2v* m, uint32_t max_batch, uint32_t max_wait_us) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    m->coalescer.configure(max_batch, max_wait_us);
    return FSGPU_OK;
}

fsgpu_status fsgpu_bert_create(int32_t device, const fsgpu_bert_config* config, const fsgpu_bert_weights* weights,
                               fsgpu_bert** out) {
    if (!out || !config || !weights) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_bert();
        fsgpu::SearchError e = h->impl.init(device, *config, *weights);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_bert_create_safetensors(int32_t device, const void* blob, uint64_t blob_len, float ln_eps, fsgpu_bert** out) {
    if (!out || !blob) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_bert>();
        // the blob first (a malformed model file is reported as such on any host), then the device
        fsgpu::SearchError e = h->impl.init_safetensors(-1, blob, blob_len, ln_eps);
        if (!e.ok()) return finish(e);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        e = h->impl.init_safetensors(device, blob, blob_len, ln_eps);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

namespace {
// fsgpu_bert_options: NULL = f16; a known format and zero reserved words, else FSGPU_ERR_INVALID_CONFIG
fsgpu_status bert_linear_format(const fsgpu_bert_options* options, uint32_t* format) {
    *format = FSGPU_BERT_LINEAR_F16;
    if (!options) return FSGPU_OK;
    for (uint32_t r : options->reserved)
        if (r != 0) return fail(FSGPU_ERR_INVALID_CONFIG, "fsgpu_bert_options: reserved words must be 0");
    if (options->linear_format != FSGPU_BERT_LINEAR_F16 && options->linear_format != FSGPU_BERT_LINEAR_INT8_DYNAMIC)
        return fail(FSGPU_ERR_INVALID_CONFIG, "fsgpu_bert_options: unknown linear_format");
    *format = options->linear_format;
    return FSGPU_OK;
}
}  // namespace

fsgpu_status fsgpu_bert_create_ex(int32_t device, const fsgpu_bert_config* config, const fsgpu_bert_weights* weights,
                                  const fsgpu_bert_options* options, fsgpu_bert** out) {
    if (!out || !config || !weights) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    uint32_t format = 0;
    const fsgpu_status st = bert_linear_format(options, &format);
    if (st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        auto* h = new fsgpu_bert();
        fsgpu::SearchError e = h->impl.init(device, *config, *weights, format);
        if (!e.ok()) {
            delete h;
            return finish(e);
        }
        *out = h;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_bert_create_safetensors_ex(int32_t device, const void* blob, uint64_t blob_len, float ln_eps,
                                              const fsgpu_bert_options* options, fsgpu_bert** out) {
    if (!out || !blob) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    uint32_t format = 0;
    const fsgpu_status st = bert_linear_format(options, &format);
    if (st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_bert>();
        // the blob first (a malformed model file is reported as such on any host), then the device
        fsgpu::SearchError e = h->impl.init_safetensors(-1, blob, blob_len, ln_eps, format);
        if (!e.ok()) return finish(e);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        e = h->impl.init_safetensors(device, blob, blob_len, ln_eps, format);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

uint32_t fsgpu_bert_linear_format(const fsgpu_bert* m) { return m ? m->impl.linear_format() : FSGPU_BERT_LINEAR_F16; }

void fsgpu_bert_destroy(fsgpu_bert* m) { delete m; }

fsgpu_status fsgpu_lab_linear_int8_dynamic(int32_t device, const float* x, const float* w, const float* bias, uint32_t m, uint32_t n,
                                           uint32_t k, float* y) {
    if ((m && (!x || !y)) || !w || !bias) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (!fsgpu::bert_i8_gemm_supported((int)n, (int)k) || n > (1u << 20) || k > (1u << 20))
        return fail(FSGPU_ERR_INVALID_CONFIG, "int8 linear: K and N must be multiples of 64");
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        if (m == 0) return FSGPU_OK;
        fsgpu::DeviceBuffer dx, dw, db, dy, qx, sx, wp, sw;
        fsgpu::SearchError e = dx.reserve((size_t)m * k * 4);
        if (e.ok()) e = dw.reserve((size_t)n * k * 4);
        if (e.ok()) e = db.reserve((size_t)n * 4);
        if (e.ok()) e = dy.reserve((size_t)m * n * 4);
        if (e.ok()) e = qx.reserve((size_t)m * k);
        if (e.ok()) e = sx.reserve((size_t)m * 4);
        if (e.ok()) e = wp.reserve(fsgpu::bert_i8_packed_bytes((int)n, (int)k));
        if (e.ok()) e = sw.reserve((size_t)n * 4);
        hipError_t he = hipSuccess;
        if (e.ok()) {
            he = hipMemcpy(dx.ptr, x, (size_t)m * k * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(dw.ptr, w, (size_t)n * k * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(db.ptr, bias, (size_t)n * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_pack_w(static_cast<const float*>(dw.ptr), wp.ptr, static_cast<float*>(sw.ptr), (int)n, (int)k, nullptr);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_quant_rows(static_cast<const float*>(dx.ptr), qx.ptr, static_cast<float*>(sx.ptr), (int)m, (int)k, nullptr);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_gemm(qx.ptr, static_cast<const float*>(sx.ptr), wp.ptr, static_cast<const float*>(sw.ptr),
                                                static_cast<const float*>(db.ptr), static_cast<float*>(dy.ptr), (int)m, (int)n, (int)k, false, nullptr);
            if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
            if (he == hipSuccess) he = hipMemcpy(y, dy.ptr, (size_t)m * n * 4, hipMemcpyDeviceToHost);
        }
        for (fsgpu::DeviceBuffer* b : {&dx, &dw, &db, &dy, &qx, &sx, &wp, &sw}) b->release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

namespace {
// Device side of fsgpu_lab_bert_stage and fsgpu_lab_bert_short_stage: uploads (as f32, as f16 through launch_bert_to_half, as
// fragment-order f16 through launch_bert_pack_w) and outputs that sit between two guard bands of 64 rows.  The first failure sticks; every later step is skipped.
struct LabStage {
    static constexpr size_t kGuardRows = 64;
    static constexpr int kGuardByte = 0xA5;
    struct Out {
        unsigned char* base = nullptr;
        size_t rows = 0, cols = 0, elem = 0;
        size_t slab_rows = 0;   // non-zero: rows is slabs x 32 workspace rows of which the first slab_rows of each slab go to the host
        bool untouched = false; // the launch must leave the whole body as it was filled (nothing goes to the host)
        void* host = nullptr;
        void* ptr() const { return base + kGuardRows * cols * elem; }
    };
    std::vector<fsgpu::DeviceBuffer> bufs;
    std::vector<Out> outs;
    fsgpu::SearchError e;
    hipError_t he = hipSuccess;
    bool guard_hit = false;

    LabStage() { bufs.reserve(64); }
    ~LabStage() {
        for (fsgpu::DeviceBuffer& b : bufs) b.release();
    }
    bool ok() const { return e.ok() && he == hipSuccess; }
    void hip(hipError_t r) {
        if (ok()) he = r;
    }
    void* alloc(size_t bytes) {
        if (!ok()) return nullptr;
        bufs.emplace_back();
        e = bufs.back().reserve(bytes ? bytes : 16);
        return e.ok() ? bufs.back().ptr : nullptr;
    }
    void* raw(const void* src, size_t bytes) {
        void* d = alloc(bytes);
        if (ok()) he = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    const float* f32(const float* src, size_t n) { return static_cast<const float*>(raw(src, n * 4)); }
    void* f16(const float* src, size_t n) {
        const float* s = f32(src, n);
        void* d = alloc(n * 2);
        if (ok()) he = fsgpu::launch_bert_to_half(s, d, n, nullptr);
        return d;
    }
    void* packed(const float* w, int N, int K) {
        void* h = f16(w, (size_t)N * K);
        void* d = alloc((size_t)N * K * 2);
        if (ok()) he = fsgpu::launch_bert_pack_w(h, d, N, K, nullptr);
        return d;
    }
    // an output of rows x cols elements of elem bytes (1: int8 codes, copied as they are, 2: f16, 4: f32) for the caller's `host`; init: f32
    // rows the kernel updates in place
    void* out(size_t rows, size_t cols, size_t elem, void* host, const float* init = nullptr) {
        Out o;
        o.rows = rows, o.cols = cols, o.elem = elem, o.host = host;
        const size_t bytes = (rows + 2 * kGuardRows) * cols * elem;
        o.base = static_cast<unsigned char*>(alloc(bytes));
        if (ok()) he = hipMemset(o.base, kGuardByte, bytes);
        if (ok() && init) he = hipMemcpy(o.ptr(), init, rows * cols * elem, hipMemcpyHostToDevice);
        outs.push_back(o);
        return ok() ? o.ptr() : nullptr;
    }
    // an input workspace of `slabs` x 32 rows of f32 (f16: rounded on the device) whose rows m..31 hold NaN: host [slabs][m][cols]
    void* workspace(const float* src, size_t slabs, size_t m, size_t cols, bool half) {
        std::vector<float> h(slabs * 32 * cols, std::numeric_limits<float>::quiet_NaN());
        for (size_t sl = 0; sl < slabs; ++sl) std::memcpy(h.data() + sl * 32 * cols, src + sl * m * cols, m * cols * 4);
        return half ? f16(h.data(), h.size()) : const_cast<float*>(f32(h.data(), h.size()));
    }
    // the four-slab output: [slabs][32][cols] f32, all of it guard bytes beforehand; rows m..31 of each slab must keep them
    void* out_slabs(size_t slabs, size_t m, size_t cols, float* host) {
        void* p = out(slabs * 32, cols, 4, host);
        outs.back().slab_rows = m;
        return p;
    }
    // a buffer the launch is handed (or not) and must not write: guard bytes throughout, checked whole
    void* out_untouched(size_t rows, size_t cols, size_t elem) {
        void* p = out(rows, cols, elem, nullptr);
        outs.back().untouched = true;
        return p;
    }
    void collect() {
        hip(hipStreamSynchronize(nullptr));
        for (const Out& o : outs) {
            if (!ok()) return;
            const size_t band = kGuardRows * o.cols * o.elem, body = o.rows * o.cols * o.elem;
            std::vector<unsigned char> h(body + 2 * band);
            he = hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost);
            if (!ok()) return;
            for (size_t i = 0; i < band; ++i)
                if (h[i] != kGuardByte || h[band + body + i] != kGuardByte) guard_hit = true;
            if (o.untouched) {
                for (size_t i = 0; i < body; ++i)
                    if (h[band + i] != kGuardByte) guard_hit = true;
            } else if (o.slab_rows) {
                const size_t row = o.cols * o.elem;
                for (size_t sl = 0; sl < o.rows / 32; ++sl) {
                    const unsigned char* slab = h.data() + band + sl * 32 * row;
                    std::memcpy(reinterpret_cast<unsigned char*>(o.host) + sl * o.slab_rows * row, slab, o.slab_rows * row);
                    for (size_t i = o.slab_rows * row; i < 32 * row; ++i)
                        if (slab[i] != kGuardByte) guard_hit = true;
                }
            } else if (o.elem != 2) {
                std::memcpy(o.host, h.data() + band, body);
            } else {
                const _Float16* s = reinterpret_cast<const _Float16*>(h.data() + band);
                for (size_t i = 0; i < o.rows * o.cols; ++i) static_cast<float*>(o.host)[i] = (float)s[i];
            }
        }
    }
};

// offsets [n_docs + 1] from 0 to m, non-decreasing; the longest document (embed_batch's max_seq)
bool lab_offsets(const uint32_t* offsets, uint32_t n_docs, uint32_t m, uint32_t* max_seq, uint32_t* min_seq) {
    if (!offsets || n_docs == 0 || n_docs > (1u << 20) || offsets[0] != 0 || offsets[n_docs] != m) return false;
    *max_seq = 0;
    *min_seq = ~0u;
    for (uint32_t i = 0; i < n_docs; ++i) {
        if (offsets[i + 1] < offsets[i]) return false;
        const uint32_t len = offsets[i + 1] - offsets[i];
        *max_seq = std::max(*max_seq, len);
        *min_seq = std::min(*min_seq, len);
    }
    return true;
}
}  // namespace

fsgpu_status fsgpu_lab_bert_stage(int32_t device, const fsgpu_lab_bert_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_stage_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    const int M = (int)a.m, N = (int)a.n, K = (int)a.k, H = (int)a.hidden, I = (int)a.inter;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (a.m == 0 || a.m > (1u << 20)) return bad("bert stage: m must be in 1..=2^20");
    if (st > FSGPU_LAB_BERT_CLS_HEAD || form > 2) return bad("bert stage: unknown stage or form");
    static const int n_in[] = {1, 3, 6, 12, 5, 1, 5};
    const int need = n_in[st] + ((st == FSGPU_LAB_BERT_ATTENTION && form == 2) ? 1 : 0);
    for (int i = 0; i < need; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: missing input");
    if (!a.out0) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: out0 is null");
    const bool two_outs = st == FSGPU_LAB_BERT_LINEAR_LN || st == FSGPU_LAB_BERT_POST_ATTN || st == FSGPU_LAB_BERT_EMBED_LN ||
                          st == FSGPU_LAB_BERT_CLS_HEAD || (st == FSGPU_LAB_BERT_ATTENTION && form == 2);
    if (two_outs && !a.out1) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: out1 is null");
    // the encoder's own shape rule (NativeEmbedder::init); the linear stage has no hidden, the head has the reranker's rule
    if (st == FSGPU_LAB_BERT_CLS_HEAD) {
        if (form != 0 || !fsgpu::bert_rerank_supported(H)) return bad("bert stage: the head takes a hidden that is a multiple of 64 and <= 1024");
    } else if (st != FSGPU_LAB_BERT_LINEAR && (H <= 0 || H % 128 != 0 || H > 1024)) {
        return bad("bert stage: hidden must be a multiple of 128 and <= 1024");
    }
    uint32_t max_seq = 0, min_seq = 0;
    switch (st) {
        case FSGPU_LAB_BERT_ATTENTION:
            if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq) || max_seq > 512) return bad("bert stage: offsets must run from 0 to m in documents of at most 512 tokens");
            if (form == 2 && (min_seq == 0 || !fsgpu::bert_rerank_supported(H))) return bad("bert stage: the [CLS] attention takes no empty document");
            break;
        case FSGPU_LAB_BERT_LINEAR:
            if (N <= 0 || N > (1 << 20) || K <= 0 || K > (1 << 20)) return bad("bert stage: n and k must be in 1..=2^20");
            if (form == 0 ? (K % 32 != 0 || N % 64 != 0 || a.epilogue > 1) : (!fsgpu::bert_gemm_w_supported(N, K) || a.epilogue > 2))
                return bad("bert stage: linear shape or epilogue not supported by this form");
            break;
        case FSGPU_LAB_BERT_LINEAR_LN:
            if (K <= 0 || K > (1 << 20) || K % 32 != 0) return bad("bert stage: k must be a multiple of 32");
            if ((form == 0 && !fsgpu::bert_gemm_ln_supported(H)) || (form == 1 && !fsgpu::bert_gemm_ln_w_supported(H, K)))
                return bad("bert stage: linear + LayerNorm shape not supported by this form");
            break;
        case FSGPU_LAB_BERT_POST_ATTN:
            if (I <= 0 || I > (1 << 20)) return bad("bert stage: inter must be in 1..=2^20");
            if (form == 2 ? !(fsgpu::bert_gemm_ln_w_supported(H, H) && fsgpu::bert_ffn_w_supported(H, I)) : !fsgpu::bert_post_attn_w_supported(H, I))
                return bad("bert stage: post-attention shape not supported by this form");
            break;
        case FSGPU_LAB_BERT_EMBED_LN:
            if (form > 1 || a.vocab == 0 || a.max_pos == 0 || !a.ids || !a.positions || (form == 1 && (!a.types || !fsgpu::bert_rerank_supported(H))))
                return bad("bert stage: embedding needs ids, positions (and types), vocab and max_pos");
            for (uint32_t t = 0; t < a.m; ++t)
                if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos ||
                    (form == 1 && (a.types[t] < 0 || a.types[t] > 1)))
                    return bad("bert stage: token id, position or type out of range");
            break;
        case FSGPU_LAB_BERT_CLS_HEAD:
            break;
        default:
            if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq)) return bad("bert stage: offsets must run from 0 to m");
            break;
    }
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        const size_t m = a.m, h = a.hidden;
        if (st == FSGPU_LAB_BERT_ATTENTION) {
            const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
            const int heads = H / 32;
            if (form == 1) {
                const float* qkv = s.f32(a.in[0], m * 3 * h);
                void* ctx = s.out(m, h, 2, a.out0);
                if (s.ok()) s.hip(fsgpu::launch_bert_attention(qkv, offs, ctx, (int)a.n_docs, heads, H, (int)max_seq, a.scale, nullptr));
            } else if (form == 0) {
                const void* qkv = s.f16(a.in[0], m * 3 * h);
                void* ctx = s.out(m, h, 2, a.out0);
                if (s.ok()) s.hip(fsgpu::launch_bert_attention_h(qkv, offs, ctx, (int)a.n_docs, heads, H, (int)max_seq, a.scale, nullptr));
            } else {
                const void* qkv = s.f16(a.in[0], m * 3 * h);
                const float* x = s.f32(a.in[1], m * h);
                void* ctx = s.out(a.n_docs, h, 2, a.out0);
                float* x_cls = static_cast<float*>(s.out(a.n_docs, h, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_cls_attention(qkv, offs, x, ctx, x_cls, (int)a.n_docs, heads, H, a.scale, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_LINEAR) {
            const void* act = s.f16(a.in[0], m * a.k);
            const void* w = form == 0 ? s.f16(a.in[1], (size_t)a.n * a.k) : s.packed(a.in[1], N, K);
            const float* bias = s.f32(a.in[2], a.n);
            const bool half_out = a.epilogue != 0;
            void* y = s.out(m, a.n, half_out ? 2 : 4, a.out0);
            float* y32 = half_out ? nullptr : static_cast<float*>(y);
            void* y16 = half_out ? y : nullptr;
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_gemm(act, w, bias, y32, y16, M, N, K, a.epilogue == 1, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_gemm_w(act, w, bias, y32, y16, M, N, K, (int)a.epilogue, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_gemm_w_fixed(act, w, bias, y32, y16, M, N, K, (int)a.epilogue, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_LINEAR_LN) {
            const void* act = s.f16(a.in[0], m * a.k);
            const void* w = form == 1 ? s.packed(a.in[1], H, K) : s.f16(a.in[1], h * a.k);
            const float* bias = s.f32(a.in[2], h);
            const float* lnw = s.f32(a.in[4], h);
            const float* lnb = s.f32(a.in[5], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0, a.in[3]));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_gemm_ln(act, w, bias, x, x_h, lnw, lnb, M, H, K, a.eps, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_gemm_ln_w(act, w, bias, x, x_h, lnw, lnb, M, H, K, a.eps, nullptr));
            } else {
                float* tmp = static_cast<float*>(s.alloc(m * h * 4));
                if (s.ok()) s.hip(fsgpu::launch_bert_gemm(act, w, bias, tmp, nullptr, M, H, K, false, nullptr));
                if (s.ok()) s.hip(fsgpu::launch_bert_add_ln(x, tmp, lnw, lnb, x_h, M, H, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_POST_ATTN) {
            const size_t in = a.inter;
            const void* ctx = s.f16(a.in[0], m * h);
            const void* w0 = s.packed(a.in[1], H, H);
            const float* b0 = s.f32(a.in[2], h);
            const float* ln0w = s.f32(a.in[3], h);
            const float* ln0b = s.f32(a.in[4], h);
            const void* w1 = s.packed(a.in[5], I, H);
            const float* b1 = s.f32(a.in[6], in);
            const void* w2 = s.packed(a.in[7], H, I);
            const float* b2 = s.f32(a.in[8], h);
            const float* lnw = s.f32(a.in[9], h);
            const float* lnb = s.f32(a.in[10], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0, a.in[11]));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_post_attn_w(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_post_attn_w_fixed(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_gemm_ln_w(ctx, w0, b0, x, x_h, ln0w, ln0b, M, H, H, a.eps, nullptr));
                if (s.ok()) s.hip(fsgpu::launch_bert_ffn_w(w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_EMBED_LN) {
            const int32_t* ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
            const int32_t* positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
            const int32_t* types = form == 1 ? static_cast<const int32_t*>(s.raw(a.types, m * 4)) : nullptr;
            const float* word = s.f32(a.in[0], (size_t)a.vocab * h);
            const float* pos = s.f32(a.in[1], (size_t)a.max_pos * h);
            const float* type = s.f32(a.in[2], (form == 1 ? 2 : 1) * h);
            const float* lnw = s.f32(a.in[3], h);
            const float* lnb = s.f32(a.in[4], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_embed_ln(ids, positions, word, pos, type, lnw, lnb, x, x_h, M, H, a.eps, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_embed_typed_ln(ids, types, positions, word, pos, type, lnw, lnb, x, x_h, M, H, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_CLS_HEAD) {
            const float* x_cls = s.f32(a.in[0], m * h);
            const float* pool_w = s.f32(a.in[1], h * h);
            const float* pool_b = s.f32(a.in[2], h);
            const float* cls_w = s.f32(a.in[3], h);
            const float* cls_b = s.f32(a.in[4], 1);
            float* logits = static_cast<float*>(s.out(m, 1, 4, a.out0));
            float* scores = static_cast<float*>(s.out(m, 1, 4, a.out1));
            if (s.ok()) s.hip(fsgpu::launch_bert_cls_head(x_cls, pool_w, pool_b, cls_w, cls_b, logits, scores, M, H, nullptr));
        } else {
            const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
            const float* x = s.f32(a.in[0], m * h);
            float* pooled = static_cast<float*>(s.out(a.n_docs, h, 4, a.out0));
            if (s.ok()) s.hip(fsgpu::launch_bert_pool(x, offs, pooled, (int)a.n_docs, H, nullptr));
        }
        s.collect();
        if (!s.e.ok()) return finish(s.e);
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (s.guard_hit) return fail(FSGPU_ERR_DEVICE, "bert stage: a kernel wrote into a guard band of its output");
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_bert_int8_stage(int32_t device, const fsgpu_lab_bert_int8_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_int8_stage_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    const int M = (int)a.m, N = (int)a.n, K = (int)a.k, H = (int)a.hidden;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (st > FSGPU_LAB_BERT_I8_ADD_LN_QUANT) return bad("bert int8 stage: unknown stage");
    const bool two_forms = st == FSGPU_LAB_BERT_I8_QUANT_ROWS || st == FSGPU_LAB_BERT_I8_ADD_LN_QUANT;
    if (form > (two_forms ? 1u : 0u)) return bad("bert int8 stage: unknown form");
    static const int n_in[] = {1, 1, 3, 5, 4};
    for (int i = 0; i < n_in[st]; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert int8 stage: missing input");
    const bool no_q = st == FSGPU_LAB_BERT_I8_ADD_LN_QUANT && form == 1;
    const bool f32_out = st >= FSGPU_LAB_BERT_I8_GEMM, q_out = st != FSGPU_LAB_BERT_I8_GEMM && !no_q;
    if ((f32_out && !a.out_f32) || (q_out && (!a.out_codes || !a.out_scales)) || (st == FSGPU_LAB_BERT_I8_GEMM && !a.codes))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "bert int8 stage: missing output or codes");
    if (st != FSGPU_LAB_BERT_I8_PACK_W && (a.m == 0 || a.m > (1u << 20))) return bad("bert int8 stage: m must be in 1..=2^20");
    if (st <= FSGPU_LAB_BERT_I8_GEMM) {
        // 127 x 127 x K < 2^31 (the i32 accumulator): K <= 4096 here
        if (K <= 0 || K % 64 != 0 || K > 4096) return bad("bert int8 stage: k must be a multiple of 64 and <= 4096");
        if (st != FSGPU_LAB_BERT_I8_QUANT_ROWS && (a.n > (1u << 20) || !fsgpu::bert_i8_gemm_supported(N, K)))
            return bad("bert int8 stage: n must be a multiple of 64");
        if (st == FSGPU_LAB_BERT_I8_GEMM && a.epilogue > 1) return bad("bert int8 stage: unknown epilogue");
    } else {
        if (H <= 0 || H % 64 != 0 || H > 1024) return bad("bert int8 stage: hidden must be a multiple of 64 and <= 1024");
        if (st == FSGPU_LAB_BERT_I8_EMBED_LN_QUANT) {
            if (a.vocab == 0 || a.max_pos == 0 || !a.ids || !a.positions) return bad("bert int8 stage: embedding needs ids, positions, vocab and max_pos");
            for (uint32_t t = 0; t < a.m; ++t)
                if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos)
                    return bad("bert int8 stage: token id or position out of range");
        }
    }
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        const size_t m = a.m, n = a.n, k = a.k, h = a.hidden;
        if (st == FSGPU_LAB_BERT_I8_QUANT_ROWS) {
            const void* x = form == 1 ? s.f16(a.in[0], m * k) : static_cast<const void*>(s.f32(a.in[0], m * k));
            void* q = s.out(m, k, 1, a.out_codes);
            float* sc = static_cast<float*>(s.out(m, 1, 4, a.out_scales));
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_i8_quant_rows_h(x, q, sc, M, K, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_i8_quant_rows(static_cast<const float*>(x), q, sc, M, K, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_I8_PACK_W) {
            const float* w = s.f32(a.in[0], n * k);
            void* wp = s.out(n, k, 1, a.out_codes);
            float* sw = static_cast<float*>(s.out(n, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_pack_w(w, wp, sw, N, K, nullptr));
        } else if (st == FSGPU_LAB_BERT_I8_GEMM) {
            const void* qa = s.raw(a.codes, m * k);
            const float* sa = s.f32(a.in[0], m);
            const float* w = s.f32(a.in[1], n * k);
            const float* bias = s.f32(a.in[2], n);
            void* wp = s.alloc(fsgpu::bert_i8_packed_bytes(N, K));
            float* sw = static_cast<float*>(s.alloc(n * 4));
            float* y = static_cast<float*>(s.out(m, n, 4, a.out_f32));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_pack_w(w, wp, sw, N, K, nullptr));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_gemm(qa, sa, wp, sw, bias, y, M, N, K, a.epilogue == 1, nullptr));
        } else if (st == FSGPU_LAB_BERT_I8_EMBED_LN_QUANT) {
            const int32_t* ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
            const int32_t* positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
            const float* word = s.f32(a.in[0], (size_t)a.vocab * h);
            const float* pos = s.f32(a.in[1], (size_t)a.max_pos * h);
            const float* type0 = s.f32(a.in[2], h);
            const float* lnw = s.f32(a.in[3], h);
            const float* lnb = s.f32(a.in[4], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out_f32));
            void* q = s.out(m, h, 1, a.out_codes);
            float* sc = static_cast<float*>(s.out(m, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_embed_ln_quant(ids, positions, word, pos, type0, lnw, lnb, x, q, sc, M, H, a.eps, nullptr));
        } else {
            const float* delta = s.f32(a.in[1], m * h);
            const float* lnw = s.f32(a.in[2], h);
            const float* lnb = s.f32(a.in[3], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out_f32, a.in[0]));
            void* q = no_q ? s.out_untouched(m, h, 1) : s.out(m, h, 1, a.out_codes);
            float* sc = static_cast<float*>(no_q ? s.out_untouched(m, 1, 4) : s.out(m, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_add_ln_quant(x, delta, lnw, lnb, no_q ? nullptr : q, sc, M, H, a.eps, nullptr));
        }
        s.collect();
        if (!s.e.ok()) return finish(s.e);
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (s.guard_hit) return fail(FSGPU_ERR_DEVICE, "bert int8 stage: a kernel wrote into a guard band or into a buffer it must leave alone");
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_bert_short_stage(int32_t device, const fsgpu_lab_bert_short_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_short_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (st > FSGPU_LAB_BERT_DOCS) return bad("bert short stage: unknown stage");
    const bool docs = st == FSGPU_LAB_BERT_DOCS;
    if (form > (st == FSGPU_LAB_BERT_Q_ATTN ? 1u : st == FSGPU_LAB_BERT_Q_GEMM ? 2u : 0u)) return bad("bert short stage: unknown form");
    if (!(docs ? fsgpu::bert_docs_w_supported((int)a.hidden, (int)a.inter, (int)a.heads)
               : fsgpu::bert_query_path_supported((int)a.hidden, (int)a.inter, (int)a.heads)))
        return bad("bert short stage: the short-text kernels are built for hidden 384, inter 1536, 12 heads");
    const bool embeds = docs || (st == FSGPU_LAB_BERT_Q_ATTN && form == 0);
    static const int n_in[4][3] = {{7, 7, 0}, {2, 7, 2}, {5, 0, 0}, {5, 0, 0}};
    for (int i = 0; i < n_in[st][form]; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: missing input");
    if (!a.out0) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: out0 is null");
    const bool two_outs = st == FSGPU_LAB_BERT_Q_ATTN || (st == FSGPU_LAB_BERT_Q_GEMM && form == 1);
    if (two_outs && !a.out1) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: out1 is null");
    if (a.m == 0 || a.m > (docs ? (1u << 20) : 32u)) return bad("bert short stage: m must be in 1..=32 (DOCS: 1..=2^20)");
    uint32_t max_seq = 0, min_seq = 0;
    if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq)) return bad("bert short stage: offsets must run from 0 to m");
    if (docs && (max_seq > 32 || a.layers == 0 || a.layers > 6)) return bad("bert short stage: DOCS takes texts of at most 32 tokens and 1..=6 layers");
    if (docs) {
        if (!a.layer_in) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: layer_in is null");
        for (uint32_t i = 0; i < a.layers * 12; ++i)
            if (!a.layer_in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: missing layer tensor");
    }
    if (embeds) {
        if (!a.ids || (!docs && !a.positions) || a.vocab == 0 || a.max_pos == 0 || a.max_pos > 512)
            return bad("bert short stage: embedding needs ids (, positions), vocab and max_pos in 1..=512");
        for (uint32_t t = 0; t < a.m; ++t)
            if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || (!docs && (a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos)))
                return bad("bert short stage: token id or position out of range");
        if (docs && max_seq > a.max_pos) return bad("bert short stage: text longer than max_pos");
    }
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        const size_t m = a.m, H = a.hidden, I = a.inter;
        const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
        if (!docs) {
            // the argument block as NativeEmbedder::forward_query fills it
            fsgpu::BertQueryArgs q{};
            q.tokens = (int)a.m;
            q.n_docs = (int)a.n_docs;
            q.offsets = offs;
            q.eps = a.eps;
            q.attn_scale = a.scale;
            // the pending add + LayerNorm of `slabs` partial slabs: in[0..4]
            auto pending = [&](int slabs) {
                q.x_in = static_cast<const float*>(s.workspace(a.in[0], 1, m, H, false));
                q.parts = static_cast<const float*>(s.workspace(a.in[1], (size_t)slabs, m, H, false));
                q.n_parts = slabs;
                q.prev_bias = s.f32(a.in[2], H);
                q.lnw = s.f32(a.in[3], H);
                q.lnb = s.f32(a.in[4], H);
            };
            if (st == FSGPU_LAB_BERT_Q_ATTN) {
                if (form == 0) {
                    q.ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
                    q.positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
                    q.word = s.f32(a.in[0], (size_t)a.vocab * H);
                    q.pos = s.f32(a.in[1], (size_t)a.max_pos * H);
                    q.type0 = s.f32(a.in[2], H);
                    q.lnw = s.f32(a.in[3], H);
                    q.lnb = s.f32(a.in[4], H);
                } else {
                    pending(4);
                }
                q.w = static_cast<const _Float16*>(s.f16(a.in[5], 3 * H * H));
                q.ldw = (int)H;
                q.bias = s.f32(a.in[6], 3 * H);
                q.out_h = static_cast<_Float16*>(s.out(m, H, 2, a.out0));
                q.x_out = static_cast<float*>(s.out(m, H, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_qkv_attn(q, (int)a.heads, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM && form == 0) {
                q.a_h = static_cast<const _Float16*>(s.workspace(a.in[0], 1, m, H, true));
                q.lda = (int)H;
                q.w = static_cast<const _Float16*>(s.f16(a.in[1], H * H));
                q.ldw = (int)H;
                q.n = (int)H;
                q.out_f32 = static_cast<float*>(s.out(m, H, 4, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 0, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM && form == 1) {
                pending(1);
                q.w = static_cast<const _Float16*>(s.f16(a.in[5], I * H));
                q.ldw = (int)H;
                q.n = (int)I;
                q.bias = s.f32(a.in[6], I);
                q.out_h = static_cast<_Float16*>(s.out(m, I, 2, a.out0));
                q.x_out = static_cast<float*>(s.out(m, H, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 1, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM) {
                q.a_h = static_cast<const _Float16*>(s.workspace(a.in[0], 1, m, I, true));
                q.lda = (int)I;
                q.w = static_cast<const _Float16*>(s.f16(a.in[1], H * I));
                q.ldw = (int)I;
                q.n = (int)H;
                q.out_f32 = static_cast<float*>(s.out_slabs(4, m, H, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 2, nullptr));
            } else {
                pending(4);
                float* pooled = static_cast<float*>(s.out(a.n_docs, H, 4, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_pool(q, pooled, nullptr));
            }
        } else {
            // the argument block as NativeEmbedder::embed_docs fills it, over the embedder's own row blocks
            const fsgpu::BertDocsPacking pk = fsgpu::bert_docs_pack(a.ids, a.offsets, a.n_docs, a.m);
            std::vector<unsigned char> host(pk.in_bytes);
            pk.fill(host.data(), a.offsets);
            fsgpu::BertDocsArgs d{};
            pk.point(d, static_cast<const unsigned char*>(s.raw(host.data(), host.size())));
            d.word = s.f32(a.in[0], (size_t)a.vocab * H);
            d.pos = s.f32(a.in[1], (size_t)a.max_pos * H);
            d.type0 = s.f32(a.in[2], H);
            d.emb_lnw = s.f32(a.in[3], H);
            d.emb_lnb = s.f32(a.in[4], H);
            std::vector<fsgpu::BertDocsLayer> table(a.layers);
            for (uint32_t l = 0; l < a.layers; ++l) {
                const float* const* t = a.layer_in + (size_t)l * 12;
                fsgpu::BertDocsLayer& L = table[l];
                L.qkv_wp = s.packed(t[0], 3 * (int)H, (int)H);
                L.qkv_b = s.f32(t[1], 3 * H);
                L.ao_wp = s.packed(t[2], (int)H, (int)H);
                L.ao_b = s.f32(t[3], H);
                L.ln1_w = s.f32(t[4], H);
                L.ln1_b = s.f32(t[5], H);
                L.i_wp = s.packed(t[6], (int)I, (int)H);
                L.i_b = s.f32(t[7], I);
                L.o_wp = s.packed(t[8], (int)H, (int)I);
                L.o_b = s.f32(t[9], H);
                L.ln2_w = s.f32(t[10], H);
                L.ln2_b = s.f32(t[11], H);
            }
            d.layers = static_cast<const fsgpu::BertDocsLayer*>(s.raw(table.data(), table.size() * sizeof(fsgpu::BertDocsLayer)));
            d.nlayers = (int)a.layers;
            d.eps = a.eps;
            d.attn_scale = a.scale;
            d.out = static_cast<float*>(s.out(a.n_docs, H, 4, a.out0));
            if (s.ok()) s.hip(fsgpu::launch_bert_docs_w(d, pk.nblocks, nullptr));
        }
        s.collect();
        if (!s.e.ok()) return finish(s.e);
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (s.guard_hit) return fail(FSGPU_ERR_DEVICE, "bert short stage: a kernel wrote into a guard band of its output");
        return FSGPU_OK;
    });
}

namespace {
// What fsgpu_lab_scan_stage derives from its arguments once they have passed: queries per group, groups, row pitch, output sizes.
struct ScanStageGeom {
    uint32_t group_q = 0, groups = 1;
    bool sample = false, lists = false, counts = false;
    size_t pitch = 0, cand_n = 0, count_n = 0, spill_n = 0, dense_n = 0;
};

fsgpu_status scan_stage_check(const fsgpu_lab_scan_stage_args& a, ScanStageGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    ScanStageGeom g;
    if (a.kernel > FSGPU_LAB_SCAN_PREPARE) return bad("scan stage: unknown kernel");
    if (a.elem_bytes != 1 && a.elem_bytes != 2) return bad("scan stage: elem_bytes must be 1 or 2");
    if (a.kernel == FSGPU_LAB_SCAN_PREPARE) {
        if (a.dim == 0 || a.dim > 4096) return bad("scan stage: prepare takes dim in 1..=4096");
        if (a.nq_pad == 0 || a.nq_pad > 4096 || a.nq > a.nq_pad) return bad("scan stage: prepare takes nq <= nq_pad in 1..=4096");
        if (a.elem_bytes == 1 && a.bits != 8 && a.bits != 4) return bad("scan stage: the int8 prepare takes bits 8 or 4");
        if ((a.nq && !a.queries_f32) || !a.prepared || !a.delta) return null("scan stage: prepare needs queries_f32, prepared and delta");
        if (geom) *geom = g;
        return FSGPU_OK;
    }
    const int dim = (int)a.dim, eb = (int)a.elem_bytes;
    if (a.nrows == 0 || a.nrows > (1u << 24)) return bad("scan stage: nrows must be in 1..=2^24");
    if (a.grid == 0 || a.grid > 4096 || a.groups > 8) return bad("scan stage: grid must be in 1..=4096 and groups at most 8");
    if (a.spill_cap > (1u << 20) || a.group_count > (1u << 16) || a.side_by_side > 1 || a.reverse > 1 || a.want_counts > 1)
        return bad("scan stage: spill_cap, group_count or a flag out of range");
    g.groups = a.groups ? a.groups : 1;
    if (a.kernel == FSGPU_LAB_SCAN_LDS) {
        if (!fsgpu::scan_mfma_supported(dim)) return bad("scan stage: scan_mfma_supported refuses the dimension");
        if (a.variant > 5 || !fsgpu::scan_mfma_shape_built((int)a.variant) || (a.variant == 4 && eb != 1))
            return bad("scan stage: the shape is not compiled into this build");
        if (a.stage > 2) return bad("scan stage: the LDS-query kernel has stages 0, 1 and 2");
        if (a.want_counts || a.side_by_side) return bad("scan stage: list lengths and side-by-side groups are the register-query kernel's");
        if (a.stage != 0 && (a.slots == 0 || (int)a.slots > fsgpu::scan_mfma_max_slots((int)a.variant))) return bad("scan stage: slots beyond scan_mfma_max_slots");
        g.group_q = (uint32_t)fsgpu::scan_mfma_query_tiles((int)a.variant) * 16;
        g.sample = a.stage < 2;
        if (a.group_stride == 0) return bad("scan stage: group_stride must be at least 1");
    } else {
        if (!fsgpu::scan_wide_supported(dim, eb)) return bad("scan stage: scan_wide_supported refuses the row length");
        if (a.variant < 2 || (int)a.variant > fsgpu::scan_wide_max_query_tiles(dim, eb)) return bad("scan stage: query tiles beyond scan_wide_max_query_tiles");
        if (a.stage < 1 || a.stage > 3) return bad("scan stage: the register-query kernel has stages 1, 2 and 3");
        if (a.stage == 3 && (eb != 1 || !fsgpu::scan_wide_group_maxima_supported(dim, (int)a.variant)))
            return bad("scan stage: scan_wide_group_maxima_supported refuses the shape");
        if (a.stage == 3 && a.want_counts) return bad("scan stage: the group-maxima stage writes no lists");
        if (a.stage != 3 && (a.slots == 0 || a.slots > fsgpu::kWideSlots)) return bad("scan stage: slots beyond kWideSlots");
        g.group_q = 128 * a.variant;
        g.sample = a.stage != 2;
        if (a.stage == 2 && a.group_count != 0) return bad("scan stage: the register-query main pass visits every row (group_count must be 0)");
        // (the kernel's list offsets are 32-bit byte offsets inside a group's lists)
        if ((uint64_t)g.group_q * a.grid * (a.stage == 3 ? 4 : a.slots) * 8 > 0xffffffffull) return bad("scan stage: a group's lists exceed 4 GB");
    }
    if (g.sample) {
        if (a.group_count == 0 || a.group_stride == 0) return bad("scan stage: a sample stage needs group_count and group_stride");
        if ((uint64_t)(a.group_count - 1) * a.group_stride * 64 >= a.nrows) return bad("scan stage: a sample group begins past the last row");
    }
    if (a.nq_pad != g.groups * g.group_q) return bad("scan stage: nq_pad must be groups x the kernel's query group");
    g.pitch = a.row_stride ? a.row_stride : (size_t)dim * eb;
    if (g.pitch < (size_t)dim * eb || (g.pitch & 15) || g.pitch > (1u << 16)) return bad("scan stage: row_stride must be a multiple of 16 bytes that holds a row");
    if ((uint64_t)a.nrows * g.pitch > (1ull << 31)) return bad("scan stage: the slab exceeds 2 GB");
    const bool gmax = a.kernel == FSGPU_LAB_SCAN_REG && a.stage == 3;
    const bool dense = a.kernel == FSGPU_LAB_SCAN_LDS && a.stage == 0;
    g.lists = !dense && !gmax;
    g.counts = a.want_counts != 0;
    g.cand_n = dense ? 0 : (size_t)a.nq_pad * a.grid * (gmax ? 4 : a.slots);
    g.count_n = g.counts ? (size_t)a.nq_pad * a.grid : 0;
    g.spill_n = g.lists ? (size_t)a.nq_pad * a.spill_cap : 0;
    g.dense_n = dense ? (size_t)a.nq_pad * a.group_count * 64 : 0;
    if ((g.cand_n | g.dense_n) > (1ull << 28)) return bad("scan stage: an output exceeds 2 GB");
    if (!a.slab || !a.queries) return null("scan stage: slab or queries is null");
    if (!dense && !gmax && !a.tau) return null("scan stage: tau is null");
    if (dense ? !a.dense : !a.cand) return null("scan stage: the stage's output is null");
    if (g.lists && (!a.spill_count || !a.overflow || (a.spill_cap && !a.spill))) return null("scan stage: spill, spill_count or overflow is null");
    if (g.counts && !a.cand_count) return null("scan stage: cand_count is null");
    if (geom) *geom = g;
    return FSGPU_OK;
}
}  // namespace

fsgpu_status fsgpu_lab_scan_stage_check(const fsgpu_lab_scan_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return scan_stage_check(*args, nullptr);
}

int32_t fsgpu_lab_scan_planner_shape(int32_t requested, int32_t elem_bytes) { return fsgpu::scan_mfma_planner_shape(requested, elem_bytes); }

fsgpu_status fsgpu_lab_scan_stage(int32_t device, const fsgpu_lab_scan_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_scan_stage_args& a = *args;
    ScanStageGeom g;
    if (const fsgpu_status st = scan_stage_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        // outputs: [band | body | band], the bands of kGuardByte, the body prefilled with `fill`
        constexpr size_t kBand = 4096;
        struct Out {
            unsigned char* base;
            size_t bytes;
            void* host;
        };
        std::vector<Out> outs;
        auto out = [&](size_t bytes, int fill, void* host) -> void* {
            if (bytes == 0 || !host) return nullptr;
            unsigned char* base = static_cast<unsigned char*>(s.alloc(bytes + 2 * kBand));
            if (s.ok()) s.hip(hipMemset(base, LabStage::kGuardByte, bytes + 2 * kBand));
            if (s.ok()) s.hip(hipMemset(base + kBand, fill, bytes));
            outs.push_back({base, bytes, host});
            return s.ok() ? base + kBand : nullptr;
        };
        if (a.kernel == FSGPU_LAB_SCAN_PREPARE) {
            const size_t qn = (size_t)a.nq * a.dim;
            const float* q = a.nq ? s.f32(a.queries_f32, qn) : static_cast<const float*>(s.alloc(16));
            void* prepared = out((size_t)a.nq_pad * a.dim * a.elem_bytes, 0xCD, a.prepared);
            float* delta = static_cast<float*>(out((size_t)a.nq_pad * 4, 0xCD, a.delta));
            if (a.elem_bytes == 2) {
                const unsigned int* mx = static_cast<const unsigned int*>(s.raw(&a.max_norm_bits, 4));
                if (s.ok()) s.hip(fsgpu::launch_prepare_queries(q, a.nq, a.nq_pad, a.dim, 0, mx, prepared, delta, nullptr));
            } else if (s.ok()) {
                s.hip(fsgpu::launch_prepare_queries_i8(q, a.nq, a.nq_pad, a.dim, prepared, delta, nullptr, (int)a.bits));
            }
        } else {
            // the slab, with guard rows behind its last row: NaN halves / 0x7f bytes
            constexpr size_t kSlabGuardRows = 256;
            const size_t body = (size_t)a.nrows * g.pitch, tail = kSlabGuardRows * g.pitch;
            unsigned char* slab = static_cast<unsigned char*>(s.alloc(body + tail));
            if (s.ok()) s.hip(hipMemcpy(slab, a.slab, body, hipMemcpyHostToDevice));
            if (s.ok()) {
                std::vector<unsigned char> guard(tail, 0x7f);
                if (a.elem_bytes == 2)
                    for (size_t i = 0; i < tail; i += 2) guard[i] = 0x00, guard[i + 1] = 0x7e;
                s.hip(hipMemcpy(slab + body, guard.data(), tail, hipMemcpyHostToDevice));
            }
            const size_t words = ((size_t)a.nrows + 63) / 64;
            auto bitmap = [&](const uint64_t* src) -> const fsgpu::u64* {
                if (!src) return nullptr;
                std::vector<uint64_t> w(words + 2, 0);   // (two zero words behind the last)
                std::memcpy(w.data(), src, words * 8);
                return static_cast<const fsgpu::u64*>(s.raw(w.data(), w.size() * 8));
            };
            fsgpu::MfmaScanArgs m{};
            m.slab = slab;
            m.live = bitmap(a.live);
            m.allow = bitmap(a.allow);
            m.queries = s.raw(a.queries, (size_t)a.nq_pad * a.dim * a.elem_bytes);
            if (a.tau) m.tau = static_cast<const float*>(s.raw(a.tau, (size_t)a.nq_pad * 4));
            m.cand = static_cast<fsgpu::u64*>(out(g.cand_n * 8, 0xCD, a.cand));
            m.cand_count = static_cast<uint32_t*>(out(g.count_n * 4, 0xCD, a.cand_count));
            m.dense = static_cast<fsgpu::u64*>(out(g.dense_n * 8, 0xCD, a.dense));
            if (g.lists) {
                m.spill = static_cast<fsgpu::u64*>(out(g.spill_n * 8, 0xCD, a.spill));
                m.spill_count = static_cast<uint32_t*>(out((size_t)a.nq_pad * fsgpu::kMfmaSpillCountStride * 4, 0, a.spill_count));
                m.overflow = static_cast<uint32_t*>(out((size_t)a.nq_pad * 4, 0, a.overflow));
            }
            m.spill_cap = a.spill_cap;
            m.nrows = a.nrows;
            m.stage = a.stage;
            m.group_stride = a.group_stride;
            m.group_count = a.group_count;
            m.dim = a.dim;
            m.slots = a.kernel == FSGPU_LAB_SCAN_REG && a.stage == 3 ? 4 : a.slots;
            m.row_base = a.row_base;
            m.elem_bytes = a.elem_bytes;
            m.reverse = a.reverse;
            m.row_stride = a.row_stride;
            m.groups = a.groups;
            m.side_by_side = a.side_by_side;
            if (s.ok()) {
                if (a.kernel == FSGPU_LAB_SCAN_LDS) s.hip(fsgpu::launch_scan_mfma(m, (int)a.variant, (int)a.grid, nullptr, nullptr));
                else s.hip(fsgpu::launch_scan_wide(m, (int)a.variant, (int)a.grid, nullptr, nullptr));
            }
        }
        s.hip(hipStreamSynchronize(nullptr));
        bool guard_hit = false;
        for (const Out& o : outs) {
            if (!s.ok()) break;
            std::vector<unsigned char> h(o.bytes + 2 * kBand);
            s.hip(hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost));
            if (!s.ok()) break;
            for (size_t i = 0; i < kBand; ++i)
                if (h[i] != LabStage::kGuardByte || h[kBand + o.bytes + i] != LabStage::kGuardByte) guard_hit = true;
            std::memcpy(o.host, h.data() + kBand, o.bytes);
        }
        if (!s.e.ok()) return finish(s.e);
        if (s.he == hipErrorInvalidValue) return fail(FSGPU_ERR_INVALID_CONFIG, "scan stage: the launcher refused the shape");
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (guard_hit) return fail(FSGPU_ERR_DEVICE, "scan stage: a kernel wrote into a guard band of its output");
        return FSGPU_OK;
    });
}

namespace {
// What fsgpu_lab_select derives from its arguments once they have passed: array sizes in elements.
struct SelectGeom {
    size_t lists_n = 0, exact_n = 0, counts_n = 0, query_rows = 0, query_pitch = 0, slab_pitch = 0, bitmap_words = 0;
    bool finish = false;
};

fsgpu_status select_check(const fsgpu_lab_select_args& a, SelectGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    SelectGeom g;
    if (a.kernel > FSGPU_LAB_TWO_PASS_MERGE) return bad("select: unknown kernel");
    if (a.kernel != FSGPU_LAB_LIST_CUT && (a.nq == 0 || a.nq > 4096)) return bad("select: nq must be in 1..=4096");
    if (a.valid_queries > a.nq) return bad("select: valid_queries beyond nq");
    if (a.dim > 4096 || a.nrows > (1u << 22) || a.spill_cap > (1u << 20) || a.extra_len > (1u << 20) || a.out_stride > 4096 || a.cand_out_stride > 4096)
        return bad("select: dim, nrows, spill_cap, extra_len or an output stride out of range");
    if (a.reset_spill > 1 || a.big_pool > 2 || a.hreduce < 0 || a.hreduce > 2) return bad("select: a flag out of range");
    // the slab and the queries of a re-score (SELECT's finish, the anchored SELECT_GROUPS)
    auto rescore_geom = [&](bool strided) -> fsgpu_status {
        const size_t elem = a.slab_f32 ? 4 : 2;
        g.slab_pitch = strided && a.row_stride ? a.row_stride : (size_t)a.dim * elem;
        if (a.dim == 0 || a.nrows == 0) return bad("select: a re-score needs dim and nrows");
        if (g.slab_pitch < (size_t)a.dim * elem || (g.slab_pitch & 15) || g.slab_pitch > (1u << 16)) return bad("select: row_stride must be a multiple of 16 bytes that holds a row");
        if ((uint64_t)a.nrows * g.slab_pitch > (1ull << 30)) return bad("select: the slab exceeds 1 GB");
        g.query_pitch = a.query_stride ? a.query_stride : a.dim;
        if (g.query_pitch < a.dim) return bad("select: query_stride below dim");
        g.query_rows = a.valid_queries ? a.valid_queries : a.nq;
        g.bitmap_words = ((size_t)a.nrows + 63) / 64;
        if (!a.queries) return null("select: queries is null");
        return FSGPU_OK;
    };
    if (a.kernel == FSGPU_LAB_SELECT) {
        fsgpu::SelectArgs s{};
        s.nlists = a.nlists, s.list_len = a.list_len, s.k = a.k, s.k_out = a.k_out, s.dim = a.dim, s.row_stride = a.row_stride, s.slab_f32 = a.slab_f32;
        s.delta = a.delta, s.slab = a.slab;
        if (!a.delta) return null("select: delta is null");
        if (!fsgpu::select_args_ok(s)) return bad("select: launch_select refuses the arguments");
        const uint64_t need = a.nlists && a.list_len ? (uint64_t)(a.nlists - 1) * a.l_stride + a.list_len : 0;
        if (a.l_stride < a.list_len || a.q_stride < need || (uint64_t)a.nq * a.q_stride > (1ull << 25)) return bad("select: q_stride / l_stride do not hold the lists, or they exceed 2^25 entries");
        if ((uint64_t)a.nlists * a.list_len + a.extra_len + a.spill_cap > (1u << 22)) return bad("select: more than 2^22 entries per query");
        g.lists_n = (size_t)a.nq * a.q_stride;
        g.counts_n = (size_t)a.nq * a.nlists;
        if (need && !a.lists) return null("select: lists is null");
        if (a.extra_len && !a.extra) return null("select: extra is null");
        if (a.spill && !a.spill_count) return null("select: spill without spill_count");
        if (a.reset_spill && !a.spill_count) return null("select: reset_spill without spill_count");
        if (a.big_pool && !a.pool_flag) return null("select: the big-pool forms need pool_flag");
        g.finish = a.slab != nullptr;
        if (g.finish) {
            if (const fsgpu_status st = rescore_geom(true); st != FSGPU_OK) return st;
            if (a.out_stride < a.k_out) return bad("select: out_stride below k_out");
            if ((a.cand_approx_out || a.cand_exact_out) && a.cand_out_stride < a.k) return bad("select: cand_out_stride below k");
        } else if (a.big_pool || a.anchor_unit || a.out_rows || a.out_scores || a.out_packed || a.out_counts || a.cand_approx_out || a.cand_exact_out) {
            return bad("select: a finish field without a slab");
        }
    } else if (a.kernel == FSGPU_LAB_SELECT_GROUPS) {
        fsgpu::GroupSelectArgs s{};
        s.nentries = a.nentries, s.k = a.k, s.dim = a.dim, s.rank_only = a.rank_only;
        s.delta = a.delta, s.tau_out = a.tau_out, s.anchor_unit = a.anchor_unit, s.slab = a.slab;
        if (!a.delta || !a.tau_out) return null("select: delta or tau_out is null");
        if (!a.rank_only && (!a.anchor_unit || !a.slab)) return null("select: the anchored form needs anchor_unit and slab");
        if (!fsgpu::select_groups_args_ok(s)) return bad("select: launch_select_groups refuses the arguments");
        if (!a.lists) return null("select: lists is null");
        if (a.reset_spill && !a.spill_count) return null("select: reset_spill without spill_count");
        g.lists_n = (size_t)a.nq * a.nentries;
        g.finish = !a.rank_only;
        if (g.finish)
            if (const fsgpu_status st = rescore_geom(false); st != FSGPU_OK) return st;
    } else if (a.kernel == FSGPU_LAB_LIST_CUT) {
        if (!fsgpu::list_cut_args_ok(a.nlists, a.list_len)) return bad("select: launch_list_cut refuses the arguments");
        if ((uint64_t)a.nlists * a.list_len > (1ull << 25)) return bad("select: the lists exceed 2^25 entries");
        g.lists_n = (size_t)a.nlists * a.list_len;
        if ((g.lists_n && !a.lists) || !a.tau_out) return null("select: lists or tau_out is null");
    } else {
        if (!fsgpu::two_pass_merge_args_ok(a.nshards, a.cc, a.k)) return bad("select: launch_two_pass_merge refuses the arguments");
        if (a.nshards == 0 || a.shard_pitch < (uint64_t)a.nq * a.cc || (uint64_t)a.nshards * a.shard_pitch > (1ull << 25)) return bad("select: shard_pitch does not hold nq x cc entries, or the lists exceed 2^25");
        g.lists_n = g.exact_n = (size_t)a.nshards * a.shard_pitch;
        if (!a.lists || !a.exact_lists) return null("select: lists or exact_lists is null");
    }
    if (geom) *geom = g;
    return FSGPU_OK;
}
}  // namespace

fsgpu_status fsgpu_lab_select_check(const fsgpu_lab_select_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return select_check(*args, nullptr);
}

fsgpu_status fsgpu_lab_select(int32_t device, const fsgpu_lab_select_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_select_args& a = *args;
    SelectGeom g;
    if (const fsgpu_status st = select_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        // outputs: [band | body | band], the bands of kGuardByte; the body prefilled with `fill`, or with the caller's contents (init)
        constexpr size_t kBand = 4096;
        struct Out {
            unsigned char* base;
            size_t bytes;
            void* host;
        };
        std::vector<Out> outs;
        auto out = [&](size_t bytes, int fill, void* host, bool init = false) -> void* {
            if (bytes == 0 || !host) return nullptr;
            unsigned char* base = static_cast<unsigned char*>(s.alloc(bytes + 2 * kBand));
            if (s.ok()) s.hip(hipMemset(base, LabStage::kGuardByte, bytes + 2 * kBand));
            if (s.ok()) s.hip(init ? hipMemcpy(base + kBand, host, bytes, hipMemcpyHostToDevice) : hipMemset(base + kBand, fill, bytes));
            outs.push_back({base, bytes, host});
            return s.ok() ? base + kBand : nullptr;
        };
        auto in_u64 = [&](const uint64_t* src, size_t n) -> const fsgpu::u64* {
            return src && n ? static_cast<const fsgpu::u64*>(s.raw(src, n * 8)) : static_cast<const fsgpu::u64*>(s.alloc(16));
        };
        auto in_f32 = [&](const float* src, size_t n) -> const float* { return src && n ? s.f32(src, n) : nullptr; };
        // the slab with NaN guard rows behind its last row, the queries with NaN rows behind the last valid one
        constexpr size_t kGuardRows = 64;
        auto nan_tail = [&](const void* src, size_t body, size_t tail, bool half) -> void* {
            std::vector<unsigned char> h(body + tail);
            std::memcpy(h.data(), src, body);
            if (half)   // f16 0x7e00
                for (size_t i = body; i + 1 < body + tail; i += 2) h[i] = 0x00, h[i + 1] = 0x7e;
            else        // f32 0x7fc00000
                for (size_t i = body; i + 3 < body + tail; i += 4) h[i] = 0, h[i + 1] = 0, h[i + 2] = 0xc0, h[i + 3] = 0x7f;
            return s.raw(h.data(), h.size());
        };
        const void* slab = nullptr;
        const float* queries = nullptr;
        const fsgpu::u64 *live = nullptr, *allow = nullptr;
        if (g.finish) {
            slab = nan_tail(a.slab, (size_t)a.nrows * g.slab_pitch, kGuardRows * g.slab_pitch, !a.slab_f32);
            queries = static_cast<const float*>(nan_tail(a.queries, g.query_rows * g.query_pitch * 4, kGuardRows * g.query_pitch * 4, false));
            auto bitmap = [&](const uint64_t* src) -> const fsgpu::u64* {
                if (!src) return nullptr;
                std::vector<uint64_t> w(g.bitmap_words + 2, 0);   // (two zero words behind the last)
                std::memcpy(w.data(), src, g.bitmap_words * 8);
                return static_cast<const fsgpu::u64*>(s.raw(w.data(), w.size() * 8));
            };
            live = bitmap(a.live);
            allow = bitmap(a.allow);
        }
        const fsgpu::u64* lists = in_u64(a.lists, g.lists_n);
        uint32_t* spill_count = static_cast<uint32_t*>(out((size_t)a.nq * fsgpu::kMfmaSpillCountStride * 4, 0, a.spill_count, true));
        float* tau_out = static_cast<float*>(out((a.kernel == FSGPU_LAB_LIST_CUT ? 1 : (size_t)a.nq) * 4, 0xCD, a.tau_out));
        uint32_t* overflow = static_cast<uint32_t*>(out((size_t)a.nq * 4, 0, a.overflow));
        if (a.kernel == FSGPU_LAB_SELECT) {
            fsgpu::SelectArgs m{};
            m.lists = lists;
            m.q_stride = a.q_stride;
            m.l_stride = a.l_stride, m.nlists = a.nlists, m.list_len = a.list_len;
            m.list_counts = a.list_counts && g.counts_n ? static_cast<const uint32_t*>(s.raw(a.list_counts, g.counts_n * 4)) : nullptr;
            m.extra = a.extra_len ? in_u64(a.extra, (size_t)a.nq * a.extra_len) : nullptr;
            m.extra_len = a.extra_len;
            m.spill = a.spill ? in_u64(a.spill, (size_t)a.nq * a.spill_cap) : nullptr;
            m.spill_count = spill_count;
            m.spill_cap = a.spill_cap;
            m.k = a.k;
            m.spill_reset = a.reset_spill ? spill_count : nullptr;
            m.delta = in_f32(a.delta, a.nq);
            m.tau_out = tau_out;
            m.pool_out = static_cast<fsgpu::u64*>(out((size_t)a.nq * fsgpu::kSelectPool * 8, 0xCD, a.pool_out));
            m.cand_counts = static_cast<uint32_t*>(out((size_t)a.nq * 4, 0xCD, a.cand_counts));
            m.overflow = overflow;
            m.take_topk = a.take_topk;
            m.anchor_unit = in_f32(a.anchor_unit, a.nq);
            m.heur_rank = a.heur_rank;
            m.tau_floor_out = static_cast<float*>(out((size_t)a.nq * 4, 0xCD, a.tau_floor_out));
            m.tau_floor_in = in_f32(a.tau_floor_in, a.nq);
            m.pool_flag = static_cast<uint32_t*>(out((size_t)a.nq * 4, 0, a.pool_flag, true));
            m.slab = slab;
            m.queries = queries;
            m.dim = a.dim, m.nrows = a.nrows, m.row_base = a.row_base, m.row_stride = a.row_stride, m.query_stride = a.query_stride;
            m.hreduce = a.hreduce;
            m.k_out = a.k_out, m.out_stride = a.out_stride;
            m.out_rows = static_cast<uint32_t*>(out((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_rows));
            m.out_scores = static_cast<float*>(out((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_scores));
            m.out_packed = static_cast<fsgpu::u64*>(out((size_t)a.nq * a.out_stride * 8, 0xCD, a.out_packed));
            m.out_counts = static_cast<uint32_t*>(out((size_t)a.nq * 4, 0xCD, a.out_counts));
            m.cand_approx_out = static_cast<fsgpu::u64*>(out((size_t)a.nq * a.cand_out_stride * 8, 0xCD, a.cand_approx_out));
            m.cand_exact_out = static_cast<fsgpu::u64*>(out((size_t)a.nq * a.cand_out_stride * 8, 0xCD, a.cand_exact_out));
            m.cand_out_stride = a.cand_out_stride;
            m.valid_queries = a.valid_queries;
            m.slab_f32 = a.slab_f32;
            if (s.ok() && a.big_pool != 2) s.hip(fsgpu::launch_select(m, (int)a.nq, nullptr));
            if (s.ok() && a.big_pool != 0) {
                m.big_pool = 1;
                s.hip(fsgpu::launch_select(m, (int)a.nq, nullptr));
            }
        } else if (a.kernel == FSGPU_LAB_SELECT_GROUPS) {
            fsgpu::GroupSelectArgs m{};
            m.groups = lists;
            m.nentries = a.nentries;
            m.k = a.k;
            m.delta = in_f32(a.delta, a.nq);
            m.anchor_unit = in_f32(a.anchor_unit, a.nq);
            m.tau_out = tau_out;
            m.overflow = overflow;
            m.spill_reset = a.reset_spill ? spill_count : nullptr;
            m.slab = slab;
            m.live = live, m.allow = allow;
            m.queries = queries;
            m.dim = a.dim, m.nrows = a.nrows, m.row_base = a.row_base, m.query_stride = a.query_stride;
            m.hreduce = a.hreduce;
            m.valid_queries = a.valid_queries;
            m.slab_f32 = a.slab_f32;
            m.rank_only = a.rank_only;
            if (s.ok()) s.hip(fsgpu::launch_select_groups(m, (int)a.nq, nullptr));
        } else if (a.kernel == FSGPU_LAB_LIST_CUT) {
            if (s.ok()) s.hip(fsgpu::launch_list_cut(lists, a.nlists, a.list_len, tau_out, nullptr));
        } else {
            const fsgpu::u64* exact = in_u64(a.exact_lists, g.exact_n);
            uint32_t* rows = static_cast<uint32_t*>(out((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_rows));
            float* scores = static_cast<float*>(out((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_scores));
            uint32_t* counts = static_cast<uint32_t*>(out((size_t)a.nq * 4, 0xCD, a.out_counts));
            if (s.ok()) s.hip(fsgpu::launch_two_pass_merge(lists, exact, a.nshards, a.shard_pitch, a.nq, a.cc, a.k, a.out_stride, rows, scores, counts, nullptr));
        }
        s.hip(hipStreamSynchronize(nullptr));
        bool guard_hit = false;
        for (const Out& o : outs) {
            if (!s.ok()) break;
            std::vector<unsigned char> h(o.bytes + 2 * kBand);
            s.hip(hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost));
            if (!s.ok()) break;
            for (size_t i = 0; i < kBand; ++i)
                if (h[i] != LabStage::kGuardByte || h[kBand + o.bytes + i] != LabStage::kGuardByte) guard_hit = true;
            std::memcpy(o.host, h.data() + kBand, o.bytes);
        }
        if (!s.e.ok()) return finish(s.e);
        if (s.he == hipErrorInvalidValue) return fail(FSGPU_ERR_INVALID_CONFIG, "select: the launcher refused the arguments");
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (guard_hit) return fail(FSGPU_ERR_DEVICE, "select: a kernel wrote into a guard band of its output");
        return FSGPU_OK;
    });
}

namespace {
// What fsgpu_lab_lone_stage derives from its arguments once they have passed: sizes in bytes / elements.
struct LoneGeom {
    size_t row_bytes = 0, slab_pitch = 0, query_bytes = 0, bitmap_words = 0, lists_n = 0;
};

fsgpu_status lone_stage_check(const fsgpu_lab_lone_stage_args& a, LoneGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    LoneGeom g;
    if (a.kind > FSGPU_LAB_LONE_MERGE) return bad("lone: unknown kind");
    if (a.kind == FSGPU_LAB_LONE_MERGE) {
        if (a.nq == 0 || a.nq > 4096) return bad("lone: nq must be in 1..=4096");
        if (a.nlists == 0 || a.list_len == 0) return bad("lone: a merge needs nlists and list_len");
        if (a.k == 0 || a.k > 256) return bad("lone: k must be in 1..=256");
        if (a.out_stride < a.k || a.out_stride > 4096) return bad("lone: out_stride below k, or above 4096");
        if (a.lists_sorted > 1) return bad("lone: a flag out of range");
        if ((uint64_t)a.nlists * a.list_len > (1u << 22)) return bad("lone: more than 2^22 entries per query");
        const uint64_t need = (uint64_t)(a.nlists - 1) * a.l_stride + a.list_len;
        if (a.l_stride < a.list_len || a.q_stride < need || (uint64_t)a.nq * a.q_stride > (1ull << 25))
            return bad("lone: q_stride / l_stride do not hold the lists, or they exceed 2^25 entries");
        g.lists_n = (size_t)a.nq * a.q_stride;
        if (!a.lists) return null("lone: lists is null");
        if (geom) *geom = g;
        return FSGPU_OK;
    }
    const int nq = (int)a.nq, tier = (int)a.tier, dim = (int)a.dim;
    if (a.tier != 64 && a.tier != 256) return bad("lone: tier must be 64 or 256");
    if (a.k == 0 || a.k > a.tier) return bad("lone: k must be in 1..=tier");
    if (a.grid == 0 || a.grid > 4096) return bad("lone: grid must be in 1..=4096");
    if (a.nrows == 0 || a.nrows > (1u << 22)) return bad("lone: nrows must be in 1..=2^22");
    if (a.dim == 0 || a.dim > 4096 || (a.dim & 7)) return bad("lone: dim must be a multiple of 8 up to 4096");
    if (a.hreduce < 0 || a.hreduce > 2 || a.force_runtime_dim > 1 || a.plain_loads > 1) return bad("lone: a flag out of range");
    if (a.kind != FSGPU_LAB_LONE_F16 && (a.force_runtime_dim || a.plain_loads)) return bad("lone: force_runtime_dim / plain_loads are launch_scan_topk's");
    bool strided_ok = false;
    switch (a.kind) {
        case FSGPU_LAB_LONE_F16:
            if (nq != 1 && nq != 2 && nq != 4) return bad("lone: launch_scan_topk takes 1, 2 or 4 queries per pass");
            if (fsgpu::scan_lds_bytes(dim, nq, tier) > 160 * 1024) return bad("lone: the queries and lists exceed the LDS");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)nq * dim * 4, strided_ok = true;
            break;
        case FSGPU_LAB_LONE_F16_HOST_QUERY:
            if (nq != 1) return bad("lone: the host-query form takes one query");
            if (!fsgpu::scan_kernarg_query_supported(dim, tier)) return bad("lone: scan_kernarg_query_supported refuses the shape");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)dim * 4, strided_ok = true;
            break;
        case FSGPU_LAB_LONE_F16_MQ:
            if (!fsgpu::scan_mq_supported(dim, nq, tier)) return bad("lone: scan_mq_supported refuses the shape");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)nq * dim * 4;
            break;
        case FSGPU_LAB_LONE_I8:
            if (nq != 1) return bad("lone: the int8 scan takes one query");
            if (!fsgpu::scan_i8_fused_supported(dim, tier)) return bad("lone: scan_i8_fused_supported refuses the shape");
            g.row_bytes = g.query_bytes = (size_t)dim;
            break;
        case FSGPU_LAB_LONE_I4:
            if (nq != 1) return bad("lone: the 4-bit scan takes one query");
            if (!fsgpu::scan_4bit_fused_supported(dim, tier)) return bad("lone: scan_4bit_fused_supported refuses the shape");
            g.row_bytes = g.query_bytes = (size_t)dim / 2;
            break;
        default:
            if (nq != 1 && nq != 2 && nq != 4) return bad("lone: launch_scan_topk_f32 takes 1, 2 or 4 queries per pass");
            if ((size_t)nq * dim * 4 > (size_t)96 * 1024 || fsgpu::scan_lds_bytes(dim, nq, tier) > 160 * 1024)
                return bad("lone: the queries and lists exceed the LDS");
            g.row_bytes = (size_t)dim * 4, g.query_bytes = (size_t)nq * dim * 4, strided_ok = true;
            break;
    }
    g.slab_pitch = a.row_stride ? a.row_stride : g.row_bytes;
    if (g.slab_pitch < g.row_bytes || (g.slab_pitch & 15) || g.slab_pitch > (1u << 16)) return bad("lone: row_stride must be a multiple of 16 bytes that holds a row");
    if (!strided_ok && g.slab_pitch != g.row_bytes) return bad("lone: this kernel reads dense rows only");
    if ((uint64_t)a.nrows * g.slab_pitch > (1ull << 30)) return bad("lone: the slab exceeds 1 GB");
    g.bitmap_words = ((size_t)a.nrows + 63) / 64;
    if ((a.live || a.allow) && a.bitmap_words < g.bitmap_words) return bad("lone: a bitmap shorter than the rows");
    if (!a.slab || !a.queries || !a.partial) return null("lone: slab, queries or partial is null");
    if (geom) *geom = g;
    return FSGPU_OK;
}
}  // namespace

fsgpu_status fsgpu_lab_lone_stage_check(const fsgpu_lab_lone_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return lone_stage_check(*args, nullptr);
}

fsgpu_status fsgpu_lab_lone_stage(int32_t device, const fsgpu_lab_lone_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_lone_stage_args& a = *args;
    LoneGeom g;
    if (const fsgpu_status st = lone_stage_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        LabStage s;
        // outputs: [band | body | band], the bands of kGuardByte, the body of 0xCD
        constexpr size_t kBand = 4096;
        struct Out {
            unsigned char* base;
            size_t bytes;
            void* host;
        };
        std::vector<Out> outs;
        auto out = [&](size_t bytes, void* host) -> void* {
            if (bytes == 0 || !host) return nullptr;
            unsigned char* base = static_cast<unsigned char*>(s.alloc(bytes + 2 * kBand));
            if (s.ok()) s.hip(hipMemset(base, LabStage::kGuardByte, bytes + 2 * kBand));
            if (s.ok()) s.hip(hipMemset(base + kBand, 0xCD, bytes));
            outs.push_back({base, bytes, host});
            return s.ok() ? base + kBand : nullptr;
        };
        if (a.kind == FSGPU_LAB_LONE_MERGE) {
            fsgpu::MergeArgs m;
            m.lists = static_cast<const fsgpu::u64*>(s.raw(a.lists, g.lists_n * 8));
            m.q_stride = a.q_stride;
            m.l_stride = a.l_stride;
            m.nlists = a.nlists;
            m.list_len = a.list_len;
            m.k = a.k;
            m.out_stride = a.out_stride;
            m.out_rows = static_cast<uint32_t*>(out((size_t)a.nq * a.out_stride * 4, a.out_rows));
            m.out_scores = static_cast<float*>(out((size_t)a.nq * a.out_stride * 4, a.out_scores));
            m.out_counts = static_cast<uint32_t*>(out((size_t)a.nq * 4, a.out_counts));
            m.out_packed = static_cast<fsgpu::u64*>(out((size_t)a.nq * a.out_stride * 8, a.out_packed));
            m.lists_sorted = a.lists_sorted;
            if (s.ok()) s.hip(fsgpu::launch_merge_topk(m, (int)a.nq, nullptr));
        } else {
            // the slab with guard rows behind its last row: NaN (f16 0x7e00, f32 0x7fc00000) or 0x7f (int8, 4-bit)
            constexpr size_t kGuardRows = 64;
            const size_t body = (size_t)a.nrows * g.slab_pitch, tail = kGuardRows * g.slab_pitch;
            std::vector<unsigned char> h(body + tail, 0x7f);
            std::memcpy(h.data(), a.slab, body);
            if (a.kind == FSGPU_LAB_LONE_F32)
                for (size_t i = body; i + 3 < body + tail; i += 4) h[i] = 0, h[i + 1] = 0, h[i + 2] = 0xc0, h[i + 3] = 0x7f;
            else if (a.kind <= FSGPU_LAB_LONE_F16_MQ)
                for (size_t i = body; i + 1 < body + tail; i += 2) h[i] = 0x00, h[i + 1] = 0x7e;
            const void* slab = s.raw(h.data(), h.size());
            auto bitmap = [&](const uint64_t* src) -> const fsgpu::u64* {
                if (!src) return nullptr;
                std::vector<uint64_t> w(g.bitmap_words + 2, 0);   // (two zero words behind the last)
                std::memcpy(w.data(), src, g.bitmap_words * 8);
                return static_cast<const fsgpu::u64*>(s.raw(w.data(), w.size() * 8));
            };
            const bool host_query = a.kind == FSGPU_LAB_LONE_F16_HOST_QUERY;
            const void* query = host_query ? nullptr : s.raw(a.queries, g.query_bytes);
            const bool quantised = a.kind == FSGPU_LAB_LONE_I8 || a.kind == FSGPU_LAB_LONE_I4;
            fsgpu::ScanArgs m{};
            m.slab = quantised ? nullptr : slab;
            m.live = bitmap(a.live);
            m.allow = bitmap(a.allow);
            m.queries = quantised || host_query ? nullptr : static_cast<const float*>(query);
            m.partial = static_cast<fsgpu::u64*>(out((size_t)a.nq * a.grid * a.k * 8, a.partial));
            m.nrows = a.nrows;
            m.dim = a.dim;
            m.k = a.k;
            m.row_base = a.row_base;
            m.hreduce = a.hreduce;
            m.row_stride = (uint32_t)g.slab_pitch;
            const int nq = (int)a.nq, tier = (int)a.tier, grid = (int)a.grid;
            if (s.ok()) {
                switch (a.kind) {
                    case FSGPU_LAB_LONE_F16: s.hip(fsgpu::launch_scan_topk(m, nq, tier, grid, nullptr, a.force_runtime_dim != 0, a.plain_loads != 0)); break;
                    case FSGPU_LAB_LONE_F16_HOST_QUERY: s.hip(fsgpu::launch_scan_topk_host_query(m, static_cast<const float*>(a.queries), tier, grid, nullptr)); break;
                    case FSGPU_LAB_LONE_F16_MQ: s.hip(fsgpu::launch_scan_mq(m, nq, tier, grid, nullptr, nullptr)); break;
                    case FSGPU_LAB_LONE_I8: s.hip(fsgpu::launch_scan_i8(m, slab, query, tier, grid, nullptr, nullptr)); break;
                    case FSGPU_LAB_LONE_I4: s.hip(fsgpu::launch_scan_4bit(m, slab, query, tier, grid, nullptr, nullptr)); break;
                    default: s.hip(fsgpu::launch_scan_topk_f32(m, tier, nq, grid, nullptr, nullptr)); break;
                }
            }
        }
        s.hip(hipStreamSynchronize(nullptr));
        bool guard_hit = false;
        for (const Out& o : outs) {
            if (!s.ok()) break;
            std::vector<unsigned char> h(o.bytes + 2 * kBand);
            s.hip(hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost));
            if (!s.ok()) break;
            for (size_t i = 0; i < kBand; ++i)
                if (h[i] != LabStage::kGuardByte || h[kBand + o.bytes + i] != LabStage::kGuardByte) guard_hit = true;
            std::memcpy(o.host, h.data() + kBand, o.bytes);
        }
        if (!s.e.ok()) return finish(s.e);
        if (s.he == hipErrorInvalidValue) return fail(FSGPU_ERR_INVALID_CONFIG, "lone: the launcher refused the arguments");
        if (s.he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(s.he));
        if (guard_hit) return fail(FSGPU_ERR_DEVICE, "lone: a kernel wrote into a guard band of its output");
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_bert_embed_device(fsgpu_bert* m, const int32_t* ids, const uint32_t* offsets, uint32_t n, float* out_dev) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (n && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_dev is null");
    return guarded([&]() -> fsgpu_status { return finish(m->impl.embed_batch(ids, offsets, n, nullptr, out_dev)); });
}

fsgpu_status fsgpu_device_malloc(int32_t device, uint64_t bytes, void** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_NO_DEVICE, "no such HIP device");
    if (hipMalloc(out, bytes ? bytes : 1) != hipSuccess) {
        (void)hipGetLastError();
        return fail(FSGPU_ERR_DEVICE, "device allocation failed");
    }
    return FSGPU_OK;
}

fsgpu_status fsgpu_device_free(int32_t device, void* ptr) {
    if (!ptr) return FSGPU_OK;
    if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_NO_DEVICE, "no such HIP device");
    return hipFree(ptr) == hipSuccess ? FSGPU_OK : fail(FSGPU_ERR_DEVICE, "hipFree failed");
}

int32_t fsgpu_bert_device(const fsgpu_bert* m) { return m ? m->impl.device() : -1; }
int32_t fsgpu_m2v_device(const fsgpu_m2v* m) { return m ? m->impl.device() : -1; }
int32_t fsgpu_index_device(const fsgpu_index* idx) { return idx ? idx->impl.device() : -1; }

fsgpu_status fsgpu_search_topk_batched_device_queries(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                      uint32_t k, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                                      uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries_dev || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_batched(queries_dev, nq, query_len, k, nullptr, out_rows, out_scores, out_counts, out_fallbacks,
                                                     nullptr, true));
    });
}
fsgpu_status fsgpu_search_topk_int8_two_pass_batched_device_queries(fsgpu_index* idx, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                                    uint32_t k, uint32_t candidate_multiplier, uint32_t* out_rows,
                                                                    float* out_scores, uint32_t* out_counts, uint32_t* out_fallbacks) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries_dev || !out_counts || (k && (!out_rows || !out_scores)))) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.search_top_k_int8_batched(queries_dev, nq, query_len, k, candidate_multiplier, out_rows, out_scores, out_counts,
                                                          out_fallbacks, 8, true));
    });
}
uint32_t fsgpu_bert_dimension(const fsgpu_bert* m) { return m ? m->impl.dimension() : 0; }

fsgpu_status fsgpu_bert_embed(fsgpu_bert* m, const int32_t* ids, const uint32_t* offsets, uint32_t n, float* out) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (m->coalescer.enabled() && n == 1 && offsets && out && (ids || offsets[1] == offsets[0])) {
        return guarded([&]() -> fsgpu_status {
            EmbedCall<int32_t> call;
            call.ids = ids ? ids + offsets[0] : nullptr;
            call.len = offsets[1] - offsets[0];
            call.out = out;
            m->coalescer.submit(
                &call, [m](std::vector<EmbedCall<int32_t>*>& batch) { run_embed_batch(m, m->impl.dimension(), batch); },
                [](const EmbedCall<int32_t>&, const EmbedCall<int32_t>&) { return true; });
            if (call.exec_threw) return fail(FSGPU_ERR_DEVICE, "coalesced batch failed before this request was served");
            if (call.status != FSGPU_OK) g_last_error = call.detail;
            return call.status;
        });
    }
    return guarded([&]() -> fsgpu_status { return finish(m->impl.embed_batch(ids, offsets, n, out)); });
}

fsgpu_status fsgpu_bert_set_coalescing(fsgpu_bert* m, uint32_t max_batch, uint32_t max_wait_us) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    m->coalescer.configure(max_batch, max_wait_us);
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_after_enqueue_hook(fsgpu_index* idx, fsgpu_after_enqueue_fn fn, void* ctx) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.after_enqueue_fn = fn;
    idx->impl.after_enqueue_ctx = ctx;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_profiling(fsgpu_index* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.profiling = enabled != 0;
    idx->impl.profile_period = enabled > 1 ? enabled : 1;
    idx->impl.profile_tick_ = 0;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_scan_time(fsgpu_index* idx, double* total_ms, uint64_t* launches, int32_t reset) {
    if (!idx || !total_ms || !launches) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.scan_time(total_ms, launches, nullptr, reset != 0));
    });
}

fsgpu_status fsgpu_index_scan_stats(fsgpu_index* idx, double* total_ms, uint64_t* launches, uint64_t* rows, int32_t reset) {
    if (!idx || !total_ms || !launches || !rows) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.scan_time(total_ms, launches, rows, reset != 0));
    });
}

fsgpu_status fsgpu_index_filter_stats(fsgpu_index* idx, uint64_t* gathered, uint64_t* scanned) {
    if (!idx || !gathered || !scanned) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);   // no search is running on any lane
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    *gathered = idx->impl.filter_gathered;
    *scanned = idx->impl.filter_scanned;
    for (size_t i = 0; i < idx->impl.replica_count(); ++i) {
        *gathered += idx->impl.replica(i)->filter_gathered;
        *scanned += idx->impl.replica(i)->filter_scanned;
    }
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_variant(fsgpu_index* idx, int32_t variant) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.variant = variant;
    idx->impl.sync_replicas();
    return FSGPU_OK;
}


fsgpu_status fsgpu_reranker_create(int32_t device, const fsgpu_bert_config* config, const fsgpu_reranker_weights* weights,
                                   fsgpu_reranker** out) {
    if (!out || !config || !weights) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_reranker>();
        fsgpu::SearchError e = h->impl.init(device, *config, weights->bert, weights->type_vocab, weights->pooler_w, weights->pooler_b,
                                            weights->classifier_w, weights->classifier_b);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_reranker_create_safetensors(int32_t device, const void* blob, uint64_t blob_len, float ln_eps, fsgpu_reranker** out) {
    if (!out || !blob) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_reranker>();
        // the blob first (a malformed model file is reported as such on any host), then the device
        fsgpu::SearchError e = h->impl.init_safetensors(-1, blob, blob_len, ln_eps);
        if (!e.ok()) return finish(e);
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
            return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        e = h->impl.init_safetensors(device, blob, blob_len, ln_eps);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

void fsgpu_reranker_destroy(fsgpu_reranker* m) { delete m; }
int32_t fsgpu_reranker_device(const fsgpu_reranker* m) { return m ? m->impl.device() : -1; }
uint32_t fsgpu_reranker_max_length(const fsgpu_reranker* m) { return m ? m->impl.max_length() : 0; }

fsgpu_status fsgpu_reranker_score(fsgpu_reranker* m, const int32_t* ids, const int32_t* type_ids, const uint32_t* offsets, uint32_t n,
                                  float* out_logits, float* out_scores) {
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "reranker is null");
    return guarded([&]() -> fsgpu_status { return finish(m->impl.score(ids, type_ids, offsets, n, out_logits, out_scores)); });
}

// ---- the index builder (index_builder.cpp): VectorIndexWriter::write_record + finish, lib.rs:3607-3672, 3752-3943 ----

fsgpu_status fsgpu_index_builder_create(int32_t device, uint32_t dim, const char* embedder_id, const char* embedder_revision,
                                        const fsgpu_index_builder_options* options, fsgpu_index_builder** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    fsgpu::IndexBuilder::Options o;
    if (options) {   // (judged before a device is looked for)
        if (options->quantization > 1) return fail(FSGPU_ERR_INVALID_CONFIG, "quantization must be 0 (F32) or 1 (F16)");
        if (options->compaction_gen > 255) return fail(FSGPU_ERR_INVALID_CONFIG, "compaction_gen must fit in a byte");
        if (options->reject_duplicates > 1) return fail(FSGPU_ERR_INVALID_CONFIG, "reject_duplicates must be 0 or 1");
        for (uint32_t r : options->reserved)
            if (r != 0) return fail(FSGPU_ERR_INVALID_CONFIG, "reserved option words must be 0");
        o.quantization = (uint8_t)options->quantization;
        o.compaction_gen = (uint8_t)options->compaction_gen;
        o.reject_duplicates = options->reject_duplicates == 1;
        o.chunk_rows = options->chunk_rows;
        o.reserve_rows = options->reserve_rows;
    }
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_index_builder>();
        fsgpu::SearchError e = h->impl.init(device, dim, embedder_id, embedder_revision, o);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

void fsgpu_index_builder_destroy(fsgpu_index_builder* b) { delete b; }
uint64_t fsgpu_index_builder_record_count(const fsgpu_index_builder* b) { return b ? b->impl.record_count() : 0; }

fsgpu_status fsgpu_index_builder_add(fsgpu_index_builder* b, uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens,
                                     const float* vectors, uint32_t vector_len, uint64_t* out_bad_row) {
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    return guarded([&]() -> fsgpu_status {
        return finish(b->impl.add(n, doc_ids, doc_id_lens, vectors, vector_len, false, nullptr, out_bad_row));
    });
}

fsgpu_status fsgpu_index_builder_add_device(fsgpu_index_builder* b, uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens,
                                            const float* vectors_dev, uint32_t vector_len, void* hip_stream, uint64_t* out_bad_row) {
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    return guarded([&]() -> fsgpu_status {
        return finish(b->impl.add(n, doc_ids, doc_id_lens, vectors_dev, vector_len, true, static_cast<hipStream_t>(hip_stream), out_bad_row));
    });
}

fsgpu_status fsgpu_index_builder_add_bert(fsgpu_index_builder* b, fsgpu_bert* m, const int32_t* ids, const uint32_t* offsets, uint32_t n,
                                          const char* const* doc_ids, const uint32_t* doc_id_lens, uint64_t* out_bad_row) {
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    return guarded([&]() -> fsgpu_status {
        // (the call fsgpu_bert_embed_device makes, into the builder's own buffer)
        auto embed = [&](float* out_dev) { return m->impl.embed_batch(ids, offsets, n, nullptr, out_dev); };
        return finish(b->impl.add_embedded(embed, m->impl.device(), m->impl.dimension(), n, doc_ids, doc_id_lens, out_bad_row));
    });
}

fsgpu_status fsgpu_index_builder_add_m2v(fsgpu_index_builder* b, fsgpu_m2v* m, const uint32_t* ids, const uint32_t* offsets, uint32_t n,
                                         const char* const* doc_ids, const uint32_t* doc_id_lens, uint64_t* out_bad_row) {
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    if (!m) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    return guarded([&]() -> fsgpu_status {
        auto embed = [&](float* out_dev) { return m->impl.embed_batch(ids, offsets, n, nullptr, out_dev); };
        return finish(b->impl.add_embedded(embed, m->impl.device(), m->impl.dimension(), n, doc_ids, doc_id_lens, out_bad_row));
    });
}

fsgpu_status fsgpu_index_builder_finish(fsgpu_index_builder* b, const char* path, fsgpu_index** out_index, fsgpu_index_build_stats* stats) {
    if (!out_index) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_index is null");
    *out_index = nullptr;
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_index>();
        fsgpu::IndexBuilder::Stats st;
        fsgpu::SearchError e = b->impl.finish(path, &h->impl, &st);
        if (!e.ok()) return finish(e);
        if (stats) {
            stats->rows = st.rows;
            stats->chunks = st.chunks;
            stats->ingest_launches = st.ingest_launches;
            stats->permute_launches = st.permute_launches;
            stats->ingest_ms = st.ingest_ms;
            stats->sort_ms = st.sort_ms;
            stats->permute_ms = st.permute_ms;
            stats->tables_ms = st.tables_ms;
            stats->file_ms = st.file_ms;
            stats->ingest_device_ms = st.ingest_device_ms;
            stats->permute_device_ms = st.permute_device_ms;
            stats->peak_device_bytes = st.peak_device_bytes;
        }
        *out_index = h.release();
        return FSGPU_OK;
    });
}

// ---- the hash embedder (hash_embedder.cpp): HashEmbedder, crates/frankensearch-embed/src/hash_embedder.rs:201-328 ----

fsgpu_status fsgpu_hash_create(int32_t device, uint32_t dimension, int32_t algorithm, uint64_t seed, const uint8_t* alnum_bitmap_or_null,
                               fsgpu_hash** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_hash>();
        fsgpu::SearchError e = h->impl.init(device, dimension, algorithm, seed, alnum_bitmap_or_null);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

void fsgpu_hash_destroy(fsgpu_hash* h) { delete h; }
uint32_t fsgpu_hash_dimension(const fsgpu_hash* h) { return h ? h->impl.dimension() : 0; }
int32_t fsgpu_hash_device(const fsgpu_hash* h) { return h ? h->impl.device() : -1; }

fsgpu_status fsgpu_hash_embed(fsgpu_hash* h, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out,
                              uint32_t* out_token_counts_or_null, uint32_t* out_bad_text) {
    if (!h) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (n && !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    return guarded([&]() -> fsgpu_status {
        return finish(h->impl.embed_batch(text_bytes, offsets, n, out, nullptr, out_token_counts_or_null, out_bad_text));
    });
}

fsgpu_status fsgpu_hash_embed_device(fsgpu_hash* h, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out_dev,
                                     uint32_t* out_token_counts_or_null, uint32_t* out_bad_text) {
    if (!h) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    if (n && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_dev is null");
    return guarded([&]() -> fsgpu_status {
        return finish(h->impl.embed_batch(text_bytes, offsets, n, nullptr, out_dev, out_token_counts_or_null, out_bad_text));
    });
}

fsgpu_status fsgpu_lab_hash_embed_stage_ms(fsgpu_hash* h, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out,
                                           float* out_stage_ms) {
    if (!h || !out_stage_ms) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (n && !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    return guarded([&]() -> fsgpu_status {
        return finish(h->impl.embed_batch(text_bytes, offsets, n, out, nullptr, nullptr, nullptr, out_stage_ms));
    });
}

fsgpu_status fsgpu_index_builder_add_hash(fsgpu_index_builder* b, fsgpu_hash* h, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                          const char* const* doc_ids, const uint32_t* doc_id_lens, uint64_t* out_bad_row) {
    if (!b) return fail(FSGPU_ERR_NULL_ARGUMENT, "builder is null");
    if (!h) return fail(FSGPU_ERR_NULL_ARGUMENT, "embedder is null");
    return guarded([&]() -> fsgpu_status {
        // (the call fsgpu_hash_embed_device makes, into the builder's own buffer; a refused text is the call's bad row)
        auto embed = [&](float* out_dev) {
            uint32_t bad_text = fsgpu::HashEmbedder::kNoBadText;
            fsgpu::SearchError e = h->impl.embed_batch(text_bytes, offsets, n, nullptr, out_dev, nullptr, &bad_text);
            if (!e.ok() && out_bad_row && bad_text != fsgpu::HashEmbedder::kNoBadText) *out_bad_row = bad_text;
            return e;
        };
        return finish(b->impl.add_embedded(embed, h->impl.device(), h->impl.dimension(), n, doc_ids, doc_id_lens, out_bad_row));
    });
}

// ---- the WordPiece tokenizer (wordpiece.cpp): BertNormalizer -> BertPreTokenizer -> WordPiece -> [CLS] ... [SEP] ----

fsgpu_status fsgpu_wordpiece_create(int32_t device, const fsgpu_wordpiece_config* config, fsgpu_wordpiece** out) {
    if (!out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    *out = nullptr;
    if (!config) return fail(FSGPU_ERR_NULL_ARGUMENT, "config is null");
    return guarded([&]() -> fsgpu_status {
        auto h = std::make_unique<fsgpu_wordpiece>();
        fsgpu::SearchError e = h->impl.init(device, *config);
        if (!e.ok()) return finish(e);
        *out = h.release();
        return FSGPU_OK;
    });
}

void fsgpu_wordpiece_destroy(fsgpu_wordpiece* tok) { delete tok; }
int32_t fsgpu_wordpiece_device(const fsgpu_wordpiece* tok) { return tok ? tok->impl.device() : -1; }
uint32_t fsgpu_wordpiece_vocab_size(const fsgpu_wordpiece* tok) { return tok ? tok->impl.vocab_size() : 0; }

namespace {

fsgpu_status wordpiece_encode(fsgpu_wordpiece* tok, fsgpu::WordPieceTokenizer::Request r) {
    if (!tok) return fail(FSGPU_ERR_NULL_ARGUMENT, "tokenizer is null");
    return guarded([&]() -> fsgpu_status { return finish(tok->impl.encode(r)); });
}

}  // namespace

fsgpu_status fsgpu_wordpiece_encode(fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                    int32_t add_special_tokens, uint32_t max_length, uint32_t* out_ids, uint64_t ids_capacity,
                                    uint32_t* out_offsets, uint8_t* out_status, uint64_t* out_total, uint32_t* out_bad_text) {
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = text_bytes;
    r.a_offsets = offsets;
    r.n = n;
    r.add_special = add_special_tokens != 0;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.out_ids = out_ids;
    r.out_offsets = out_offsets;
    r.out_status = out_status;
    r.out_total = out_total;
    r.out_bad_text = out_bad_text;
    return wordpiece_encode(tok, r);
}

fsgpu_status fsgpu_lab_wordpiece_encode_stage_ms(fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                                 int32_t add_special_tokens, uint32_t max_length, uint32_t* out_ids, uint64_t ids_capacity,
                                                 uint32_t* out_offsets, float* out_stage_ms) {
    if (!out_stage_ms) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_stage_ms is null");
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = text_bytes;
    r.a_offsets = offsets;
    r.n = n;
    r.add_special = add_special_tokens != 0;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.out_ids = out_ids;
    r.out_offsets = out_offsets;
    r.stage_ms = out_stage_ms;
    return wordpiece_encode(tok, r);
}

fsgpu_status fsgpu_wordpiece_encode_device(fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                           int32_t add_special_tokens, uint32_t max_length, uint32_t* out_ids_dev, uint64_t ids_capacity,
                                           uint32_t* out_offsets_dev, uint8_t* out_status, uint64_t* out_total, uint32_t* out_bad_text) {
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = text_bytes;
    r.a_offsets = offsets;
    r.n = n;
    r.add_special = add_special_tokens != 0;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.device_out = true;
    r.out_ids = out_ids_dev;
    r.out_offsets = out_offsets_dev;
    r.out_status = out_status;
    r.out_total = out_total;
    r.out_bad_text = out_bad_text;
    return wordpiece_encode(tok, r);
}

fsgpu_status fsgpu_wordpiece_encode_pairs(fsgpu_wordpiece* tok, const uint8_t* a_bytes, const uint32_t* a_offsets, const uint8_t* b_bytes,
                                          const uint32_t* b_offsets, uint32_t n, uint32_t max_length, uint32_t* out_ids,
                                          uint32_t* out_type_ids, uint64_t ids_capacity, uint32_t* out_offsets, uint8_t* out_status,
                                          uint64_t* out_total, uint32_t* out_bad_text) {
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = a_bytes;
    r.a_offsets = a_offsets;
    r.b_bytes = b_bytes;
    r.b_offsets = b_offsets;
    r.n = n;
    r.pairs = true;
    r.add_special = true;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.out_ids = out_ids;
    r.out_type_ids = out_type_ids;
    r.out_offsets = out_offsets;
    r.out_status = out_status;
    r.out_total = out_total;
    r.out_bad_text = out_bad_text;
    return wordpiece_encode(tok, r);
}

fsgpu_status fsgpu_wordpiece_encode_pairs_device(fsgpu_wordpiece* tok, const uint8_t* a_bytes, const uint32_t* a_offsets,
                                                 const uint8_t* b_bytes, const uint32_t* b_offsets, uint32_t n, uint32_t max_length,
                                                 uint32_t* out_ids_dev, uint32_t* out_type_ids_dev, uint64_t ids_capacity,
                                                 uint32_t* out_offsets_dev, uint8_t* out_status, uint64_t* out_total,
                                                 uint32_t* out_bad_text) {
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = a_bytes;
    r.a_offsets = a_offsets;
    r.b_bytes = b_bytes;
    r.b_offsets = b_offsets;
    r.n = n;
    r.pairs = true;
    r.add_special = true;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.device_out = true;
    r.out_ids = out_ids_dev;
    r.out_type_ids = out_type_ids_dev;
    r.out_offsets = out_offsets_dev;
    r.out_status = out_status;
    r.out_total = out_total;
    r.out_bad_text = out_bad_text;
    return wordpiece_encode(tok, r);
}

namespace {

using WpRequest = fsgpu::WordPieceTokenizer::Request;
using WpCsr = fsgpu::WordPieceTokenizer::OwnCsr;

// what every fused text-in call checks first; FSGPU_OK: go on
fsgpu_status fused_preamble(const void* model, fsgpu_wordpiece* tok, int model_device, uint32_t* out_bad_text) {
    if (!model) return fail(FSGPU_ERR_NULL_ARGUMENT, "model is null");
    if (!tok) return fail(FSGPU_ERR_NULL_ARGUMENT, "tokenizer is null");
    if (out_bad_text) *out_bad_text = fsgpu::WordPieceTokenizer::kNoBadText;
    if (tok->impl.device() != model_device) return fail(FSGPU_ERR_INVALID_CONFIG, "the tokenizer and the model are on different devices");
    return FSGPU_OK;
}

// raw text -> the tokenizer's device CSR -> the potion kernel, which reads the ids where they lie
fsgpu_status m2v_embed_texts(fsgpu_m2v* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out,
                             float* out_dev, uint32_t* out_bad_text) {
    const fsgpu_status pre = fused_preamble(m, tok, m ? m->impl.device() : -1, out_bad_text);
    if (pre != FSGPU_OK) return pre;
    if (n == 0) return FSGPU_OK;
    if (!out && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    return guarded([&]() -> fsgpu_status {
        WpRequest r;   // encode_fast(text, false): no special tokens, no truncation
        r.a_bytes = text_bytes;
        r.a_offsets = offsets;
        r.n = n;
        r.out_bad_text = out_bad_text;
        return finish(tok->impl.encode_then(r, [&](const WpCsr& c) { return m->impl.embed_batch_device_ids(c.ids_dev, c.offsets_dev, n, out, out_dev); }));
    });
}

// ... -> the MiniLM forward over device ids ([CLS] ... [SEP], truncated to max_length)
fsgpu_status bert_embed_texts(fsgpu_bert* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                              uint32_t max_length, float* out, float* out_dev, uint32_t* out_bad_text) {
    const fsgpu_status pre = fused_preamble(m, tok, m ? m->impl.device() : -1, out_bad_text);
    if (pre != FSGPU_OK) return pre;
    if (tok->impl.vocab_size() > m->impl.vocab()) return fail(FSGPU_ERR_INVALID_CONFIG, "the tokenizer's vocabulary is larger than the model's");
    if (n == 0) return FSGPU_OK;
    if (!out && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    return guarded([&]() -> fsgpu_status {
        WpRequest r;
        r.a_bytes = text_bytes;
        r.a_offsets = offsets;
        r.n = n;
        r.add_special = true;
        r.max_length = max_length;
        r.out_bad_text = out_bad_text;
        return finish(tok->impl.encode_then(r, [&](const WpCsr& c) {
            return m->impl.embed_batch_device_ids(reinterpret_cast<const int32_t*>(c.ids_dev), c.offsets_host, n, out, out_dev);
        }));
    });
}

}  // namespace

fsgpu_status fsgpu_m2v_embed_texts(fsgpu_m2v* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                   float* out, uint32_t* out_bad_text) {
    return m2v_embed_texts(m, tok, text_bytes, offsets, n, out, nullptr, out_bad_text);
}

fsgpu_status fsgpu_m2v_embed_texts_device(fsgpu_m2v* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                          float* out_dev, uint32_t* out_bad_text) {
    return m2v_embed_texts(m, tok, text_bytes, offsets, n, nullptr, out_dev, out_bad_text);
}

fsgpu_status fsgpu_bert_embed_texts(fsgpu_bert* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                    uint32_t max_length, float* out, uint32_t* out_bad_text) {
    return bert_embed_texts(m, tok, text_bytes, offsets, n, max_length, out, nullptr, out_bad_text);
}

fsgpu_status fsgpu_bert_embed_texts_device(fsgpu_bert* m, fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                           uint32_t max_length, float* out_dev, uint32_t* out_bad_text) {
    return bert_embed_texts(m, tok, text_bytes, offsets, n, max_length, nullptr, out_dev, out_bad_text);
}

fsgpu_status fsgpu_reranker_score_texts(fsgpu_reranker* m, fsgpu_wordpiece* tok, const uint8_t* query_bytes, uint32_t query_len,
                                        const uint8_t* doc_bytes, const uint32_t* doc_offsets, uint32_t n, uint32_t max_length,
                                        float* out_logits, float* out_scores, uint32_t* out_bad_text) {
    const fsgpu_status pre = fused_preamble(m, tok, m ? m->impl.device() : -1, out_bad_text);
    if (pre != FSGPU_OK) return pre;
    if (tok->impl.vocab_size() > m->impl.vocab()) return fail(FSGPU_ERR_INVALID_CONFIG, "the tokenizer's vocabulary is larger than the model's");
    if (m->impl.type_vocab() < 2) return fail(FSGPU_ERR_INVALID_CONFIG, "the model has no second token type for the document");
    if (n == 0) return FSGPU_OK;
    if (!out_logits || !out_scores) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_logits / out_scores is null");
    if (query_len && !query_bytes) return fail(FSGPU_ERR_NULL_ARGUMENT, "query_bytes is null");
    if ((uint64_t)query_len * n > 0xffffffffull) return fail(FSGPU_ERR_INVALID_CONFIG, "the query times the documents must stay below 4 GiB");
    return guarded([&]() -> fsgpu_status {
        // pair i is (query, document i): the query's bytes once per pair
        std::vector<uint8_t> a_bytes((size_t)query_len * n);
        std::vector<uint32_t> a_offsets((size_t)n + 1);
        for (uint32_t i = 0; i < n; ++i) {
            if (query_len) std::memcpy(a_bytes.data() + (size_t)i * query_len, query_bytes, query_len);
            a_offsets[i + 1] = (i + 1) * query_len;
        }
        fsgpu::WordPieceTokenizer::Request r;
        r.a_bytes = a_bytes.data();
        r.a_offsets = a_offsets.data();
        r.b_bytes = doc_bytes;
        r.b_offsets = doc_offsets;
        r.n = n;
        r.pairs = true;
        r.add_special = true;
        r.max_length = max_length;
        r.out_bad_text = out_bad_text;
        return finish(tok->impl.encode_then(r, [&](const fsgpu::WordPieceTokenizer::OwnCsr& c) {
            return m->impl.score_device_ids(reinterpret_cast<const int32_t*>(c.ids_dev), reinterpret_cast<const int32_t*>(c.type_ids_dev),
                                            c.offsets_host, n, out_logits, out_scores);
        }));
    });
}

}  // extern "C"

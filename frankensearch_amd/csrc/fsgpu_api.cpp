// fsgpu_api.cpp — the extern "C" boundary of libfsgpu.so (declared in include/fsgpu.h).
// Plain pointers and sizes only; every entry point catches C++ exceptions and reports a status.
#include "api_internal.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>

namespace {
thread_local std::string g_last_error;   // the one last-error string of the library (api_internal.hpp)
}  // namespace

fsgpu_status fsgpu::api::finish(const fsgpu::SearchError& e) {
    if (!e.ok()) g_last_error = e.detail;
    return e.code;
}

fsgpu_status fsgpu::api::fail(fsgpu_status code, const char* detail) {
    g_last_error = detail;
    return code;
}

using namespace fsgpu::api;

namespace {

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

void ivf_stats_out(const fsgpu::IvfStats& s, fsgpu_ivf_stats* out) {
    std::memset(out, 0, sizeof(*out));
    out->index_size = s.index_size;
    out->dimension = s.dimension;
    out->nlist = s.nlist;
    out->nprobe = s.nprobe;
    out->k_requested = s.k_requested;
    out->launches = s.launches;
    out->queries = s.queries;
    out->approximate = s.approximate;
    out->underfilled = s.underfilled;
    out->empty_despite_indexed_points = s.empty_despite_indexed_points;
    out->lists_probed = s.lists_probed;
    out->rows_scored = s.rows_scored;
    out->device_ms = s.device_ms;
}

void certified_out(const fsgpu::CertifiedEf& c, fsgpu_certified_ef* out) {
    out->ef_search = c.ef_search;
    out->meets_target = c.meets_target ? 1u : 0u;
    out->certified_recall = c.certified_recall;
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

// The two bodies a lab entry point shares with its product twin (declared in api_internal.hpp).
fsgpu_status fsgpu::api::index_query_hubness(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq, float* out,
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

fsgpu_status fsgpu::api::wordpiece_encode(fsgpu_wordpiece* tok, fsgpu::WordPieceTokenizer::Request r) {
    if (!tok) return fail(FSGPU_ERR_NULL_ARGUMENT, "tokenizer is null");
    return guarded([&]() -> fsgpu_status { return finish(tok->impl.encode(r)); });
}

extern "C" {

const char* fsgpu_version(void) { return "fsgpu 0.1.0 (gfx950)"; }

int32_t fsgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

const char* fsgpu_last_error(void) { return g_last_error.c_str(); }

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

fsgpu_status fsgpu_index_compute_query_hubness(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                               float* out) {
    return index_query_hubness(idx, queries, nq, query_dim, kq, out, nullptr);
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

// ---- the k-NN table across a rewrite or deletes (vector_index_knn_update.cpp): every refusal comes before any work ----
fsgpu_status fsgpu_knn_update_config_default(fsgpu_knn_update_config* config) {
    if (!config) return fail(FSGPU_ERR_NULL_ARGUMENT, "config is null");
    std::memset(config, 0, sizeof(*config));
    config->max_added_fraction = fsgpu::kKnnUpdDefaultMaxAddedFraction;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_update_knn_graph(fsgpu_index* idx, uint32_t m, const uint32_t* old_rows, const float* old_sims, uint64_t old_len,
                                          uint32_t old_row_base, const uint32_t* new_to_old_or_null,
                                          const fsgpu_knn_update_config* config_or_null, uint32_t* out_rows, float* out_sims,
                                          fsgpu_knn_update_stats* stats_or_null) {
    if (m < 1 || m > fsgpu::kKnnMaxM) return fail(FSGPU_ERR_INVALID_CONFIG, "m must be 1 .. 63 (k = m + 1 stays inside the fused tiers)");
    if (!old_rows || !old_sims || !out_rows || !out_sims) return fail(FSGPU_ERR_INVALID_CONFIG, "the tables and the outputs must not be null");
    if (old_len >= 0xffffffffull) return fail(FSGPU_ERR_INVALID_CONFIG, "old_len must be below 2^32 - 1: the table's ids are 32 bits wide");
    float max_added_fraction = fsgpu::kKnnUpdDefaultMaxAddedFraction;
    if (config_or_null) {
        for (uint32_t r : config_or_null->reserved)
            if (r != 0) return fail(FSGPU_ERR_INVALID_CONFIG, "the reserved words of fsgpu_knn_update_config must be 0");
        max_added_fraction = config_or_null->max_added_fraction;
    }
    if (fsgpu_device_count() <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        fsgpu::VectorIndex::KnnUpdateStats st;
        const fsgpu_status s = finish(idx->impl.update_knn_graph(m, old_rows, old_sims, old_len, old_row_base, new_to_old_or_null,
                                                                 max_added_fraction, out_rows, out_sims, &st));
        if (s == FSGPU_OK && stats_or_null) {
            std::memset(stats_or_null, 0, sizeof(*stats_or_null));
            stats_or_null->rows = st.rows;
            stats_or_null->dead = st.dead;
            stats_or_null->added = st.added;
            stats_or_null->kept_clean = st.kept_clean;
            stats_or_null->kept_dirty = st.kept_dirty;
            stats_or_null->searched_sources = st.searched_sources;
            stats_or_null->join_pairs = st.join_pairs;
            stats_or_null->join_entries = st.join_entries;
            stats_or_null->rebuilt = st.rebuilt;
            stats_or_null->device_ms = st.device_ms;
            stats_or_null->join_ms = st.join_ms;
        }
        return s;
    });
}

fsgpu_status fsgpu_index_rewrite_sources(fsgpu_index* idx, uint32_t* out_new_to_old, uint64_t* generation_before, uint64_t* generation_after,
                                         uint64_t* old_record_count) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.rewrite_sources(out_new_to_old, generation_before, generation_after, old_record_count));
    });
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

// ---- IVF index (ivf_index.cpp, ivf_kernels.hip) ----
fsgpu_status fsgpu_ivf_config_default(fsgpu_ivf_config* config) {
    if (!config) return fail(FSGPU_ERR_NULL_ARGUMENT, "config is null");
    const fsgpu::IvfConfig d;
    std::memset(config, 0, sizeof(*config));
    config->iters = d.iters;
    config->n_train = d.n_train;
    return FSGPU_OK;
}

fsgpu_status fsgpu_ivf_create(fsgpu_index* idx, uint32_t nlist, const float* init_centroids, const fsgpu_ivf_config* config, fsgpu_ivf** out) {
    if (!idx || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    *out = nullptr;
    fsgpu::IvfConfig c;
    if (config) {
        if (config->reserved0) return fail(FSGPU_ERR_INVALID_CONFIG, "reserved words of fsgpu_ivf_config must be 0");
        for (uint32_t r : config->reserved)
            if (r) return fail(FSGPU_ERR_INVALID_CONFIG, "reserved words of fsgpu_ivf_config must be 0");
        c.iters = config->iters;
        c.n_train = config->n_train;
    }
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        auto a = std::make_unique<fsgpu_ivf>();
        a->idx = idx;
        const fsgpu::SearchError e = a->impl.init(&idx->impl, nlist, init_centroids, c);
        if (!e.ok()) return finish(e);
        *out = a.release();
        return FSGPU_OK;
    });
}

void fsgpu_ivf_destroy(fsgpu_ivf* ivf) { delete ivf; }
uint64_t fsgpu_ivf_record_count(const fsgpu_ivf* ivf) { return ivf ? ivf->impl.record_count() : 0; }
int32_t fsgpu_ivf_device(const fsgpu_ivf* ivf) { return ivf ? ivf->impl.device() : -1; }
uint32_t fsgpu_ivf_nlist(const fsgpu_ivf* ivf) { return ivf ? ivf->impl.nlist() : 0; }

fsgpu_status fsgpu_ivf_centroids(fsgpu_ivf* ivf, float* out) {
    if (!ivf || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        return finish(ivf->impl.centroids(out));
    });
}

fsgpu_status fsgpu_ivf_lists(fsgpu_ivf* ivf, uint64_t* out_offsets, uint32_t* out_rows) {
    if (!ivf) return fail(FSGPU_ERR_NULL_ARGUMENT, "handle is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        return finish(ivf->impl.lists(out_offsets, out_rows));
    });
}

fsgpu_status fsgpu_ivf_build_stats(const fsgpu_ivf* ivf, fsgpu_ivf_build_info* stats) {
    if (!ivf || !stats) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu::IvfBuildStats& b = ivf->impl.build_stats();
    std::memset(stats, 0, sizeof(*stats));
    stats->iterations = b.iterations;
    stats->rows_trained = b.rows_trained;
    stats->rows_changed_last = b.rows_changed_last;
    stats->empty_lists = b.empty_lists;
    stats->largest_list = b.largest_list;
    stats->smallest_list = b.smallest_list;
    stats->assign_ms = b.assign_ms;
    stats->update_ms = b.update_ms;
    stats->lists_ms = b.lists_ms;
    return FSGPU_OK;
}

static fsgpu_status ivf_search_common(fsgpu_ivf* ivf, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe,
                                      uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* out_flags, bool on_device,
                                      fsgpu_ivf_stats* stats) {
    if (!ivf) return fail(FSGPU_ERR_NULL_ARGUMENT, "handle is null");
    if (nq && (!queries || !out_counts || !out_rows || !out_scores)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        fsgpu::IvfStats st;
        const fsgpu::SearchError e = ivf->impl.search(queries, nq, query_len, k, nprobe, out_rows, out_scores, out_counts, out_flags, on_device, &st);
        if (e.ok() && stats) ivf_stats_out(st, stats);
        return finish(e);
    });
}

fsgpu_status fsgpu_ivf_search_batched(fsgpu_ivf* ivf, const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe,
                                      uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* out_flags,
                                      fsgpu_ivf_stats* stats) {
    return ivf_search_common(ivf, queries, nq, query_len, k, nprobe, out_rows, out_scores, out_counts, out_flags, false, stats);
}

fsgpu_status fsgpu_ivf_search_batched_device_queries(fsgpu_ivf* ivf, const float* queries_dev, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t nprobe, uint32_t* out_rows_dev, float* out_scores_dev,
                                                     uint32_t* out_counts_dev, uint32_t* out_flags_dev, fsgpu_ivf_stats* stats) {
    return ivf_search_common(ivf, queries_dev, nq, query_len, k, nprobe, out_rows_dev, out_scores_dev, out_counts_dev, out_flags_dev, true, stats);
}

fsgpu_status fsgpu_ivf_search(fsgpu_ivf* ivf, const float* query, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t* out_rows,
                              float* out_scores, uint32_t* out_count, uint32_t* out_flag, fsgpu_ivf_stats* stats) {
    return ivf_search_common(ivf, query, 1, query_len, k, nprobe, out_rows, out_scores, out_count, out_flag, false, stats);
}

fsgpu_status fsgpu_ivf_last_stats(const fsgpu_ivf* ivf, fsgpu_ivf_stats* stats) {
    if (!ivf || !stats) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
    ivf_stats_out(ivf->impl.last_stats(), stats);
    return FSGPU_OK;
}

fsgpu_status fsgpu_ivf_set_list_filter(fsgpu_ivf* ivf, uint32_t mode) {
    if (!ivf) return fail(FSGPU_ERR_NULL_ARGUMENT, "handle is null");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        return finish(ivf->impl.set_list_filter(mode));
    });
}

uint32_t fsgpu_ivf_list_filter(const fsgpu_ivf* ivf) {
    if (!ivf) return 0;
    std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
    return ivf->impl.list_filter();
}

fsgpu_status fsgpu_ivf_last_filter_stats(const fsgpu_ivf* ivf, fsgpu_ivf_filter_stats* out) {
    if (!ivf || !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
    const fsgpu::IvfFilterStats s = ivf->impl.last_filter_stats();
    std::memset(out, 0, sizeof(*out));
    out->mode = s.mode;
    out->rotated = s.rotated;
    out->slot_cap = s.slot_cap;
    out->k_cap = s.k_cap;
    out->scratch_cap = s.scratch_cap;
    out->copy_bytes = s.copy_bytes;
    out->build_ms = s.build_ms;
    out->queries_filtered = s.queries_filtered;
    out->queries_uncertified = s.queries_uncertified;
    out->calls_above_k_cap = s.calls_above_k_cap;
    out->slots_filtered = s.slots_filtered;
    out->slots_overflowed = s.slots_overflowed;
    out->slots_above_scratch = s.slots_above_scratch;
    out->scratch_ranges = s.scratch_ranges;
    out->rows_filtered = s.rows_filtered;
    out->rows_rescored = s.rows_rescored;
    out->filter_ms = s.filter_ms;
    out->select_ms = s.select_ms;
    out->rescore_ms = s.rescore_ms;
    out->rows_streamed = s.rows_streamed;
    return FSGPU_OK;
}

fsgpu_status fsgpu_ivf_certify_nprobe(fsgpu_ivf* ivf, const float* queries, uint32_t nq, const uint32_t* candidate_nprobes, uint32_t n_probes,
                                      uint32_t k, double target, double alpha, fsgpu_certified_ef* chosen, fsgpu_certified_ef* sweep_out,
                                      uint32_t* n_swept) {
    if (!ivf || !chosen || !sweep_out || !n_swept || (!queries && nq) || (!candidate_nprobes && n_probes))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        std::vector<fsgpu::CertifiedEf> sweep(n_probes);
        fsgpu::CertifiedEf best;
        uint32_t swept = 0;
        const fsgpu::SearchError e = ivf->impl.certify_nprobe(queries, nq, candidate_nprobes, n_probes, k, target, alpha, &best, sweep.data(), &swept);
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

// vector_index_hits.cpp — search_hits (search_top_k + scan_wal + resolve_hits, search.rs:426-494, 1449-1475, 1493-1558) for a
// batch of queries, on the device from end to end (kernels: search_hits_kernels.hip):
//   batched search of the main rows (hits stay in HBM) | wal_topk_kernel over the WAL's device mirror -> resolve_hits_kernel -> one copy up
// Doc ids never reach the hot path: when the tables below are built the host compares them as bytes ONCE and hands the device a
// class number per main row and per WAL entry (equal ids <=> equal classes) and a bitmap of the main rows whose id has a resident
// WAL entry.  Every call that changes the WAL, the tombstones or the record table drops what it invalidates (invalidate_hits_state).
#include <unordered_map>
#include <vector>

#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

// The class of a main row is the first row with the same id bytes: rows are sorted by (FNV-1a, doc id) (lib.rs:3758-3762), so equal
// ids are adjacent.  A WAL entry takes the class of the main row with its id, live or not; an id no main row has: nrows + the first
// WAL index that carries it.
SearchError VectorIndex::ensure_hits_state() {
    FSGPU_HIP(hipSetDevice(device_));
    const size_t n = (size_t)nrows_, W = wal_.size();
    auto id_of = [&](size_t r, size_t* len) {
        *len = (size_t)(doc_offsets_[r + 1] - doc_offsets_[r]);
        return doc_blob_.data() + doc_offsets_[r];
    };
    if (!hits_main_ready_) {
        std::vector<uint32_t> cls(n);
        for (size_t r = 0; r < n; ++r) {
            cls[r] = (uint32_t)r;
            if (r == 0 || doc_hashes_[r] != doc_hashes_[r - 1]) continue;
            size_t la, lb;
            const char* a = id_of(r - 1, &la);
            const char* b = id_of(r, &lb);
            if (la == lb && std::memcmp(a, b, la) == 0) cls[r] = cls[r - 1];
        }
        FSGPU_TRY(hits_main_class_.reserve(n * 4));
        if (n) FSGPU_HIP(hipMemcpy(hits_main_class_.ptr, cls.data(), n * 4, hipMemcpyHostToDevice));
        hits_main_ready_ = true;
    }
    if (!hits_wal_ready_) {
        const size_t words = (n + 63) / 64;
        std::vector<float> mirror(W * dim_);
        std::vector<uint32_t> wcls(W);
        std::vector<uint64_t> shadow(words, 0);
        std::unordered_map<std::string, uint32_t> first;   // ids without a main row -> their first WAL index
        for (size_t w = 0; w < W; ++w) {
            const std::string& id = wal_[w].doc_id;
            std::memcpy(mirror.data() + w * dim_, wal_[w].embedding.data(), (size_t)dim_ * 4);
            const uint64_t h = fnv1a(id.data(), id.size());
            int64_t found = -1;
            auto lo = std::lower_bound(doc_hashes_.begin(), doc_hashes_.end(), h);
            for (auto it = lo; it != doc_hashes_.end() && *it == h; ++it) {
                const size_t r = (size_t)(it - doc_hashes_.begin());
                size_t len;
                const char* p = id_of(r, &len);
                if (len != id.size() || std::memcmp(p, id.data(), len) != 0) continue;
                if (found < 0) found = (int64_t)r;
                shadow[r >> 6] |= 1ull << (r & 63);   // every row of the run: live or not, best or not (search.rs:1524-1531)
            }
            wcls[w] = found >= 0 ? (uint32_t)found : first.emplace(id, (uint32_t)(n + w)).first->second;
        }
        if (W) {
            FSGPU_TRY(hits_wal_.reserve(mirror.size() * 4));
            FSGPU_TRY(hits_wal_class_.reserve(W * 4));
            FSGPU_TRY(hits_shadow_.reserve(words * 8));
            FSGPU_HIP(hipMemcpy(hits_wal_.ptr, mirror.data(), mirror.size() * 4, hipMemcpyHostToDevice));
            FSGPU_HIP(hipMemcpy(hits_wal_class_.ptr, wcls.data(), W * 4, hipMemcpyHostToDevice));
            if (words) FSGPU_HIP(hipMemcpy(hits_shadow_.ptr, shadow.data(), words * 8, hipMemcpyHostToDevice));
        }
        hits_wal_ready_ = true;
    }
    return ok();
}

// What the device path does not cover: the per-query calls, one after the other (bits = 0: search_hits; 8 / 4: the two-pass searches).
SearchError VectorIndex::hits_per_query(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t* out_rows,
                                        float* out_scores, uint32_t* out_counts, uint32_t* fallbacks, bool queries_on_device,
                                        uint32_t multiplier, int bits) {
    std::vector<float> host_copy;
    if (queries_on_device) {   // (the per-query entry points take host vectors)
        host_copy.resize((size_t)nq * dim_);
        FSGPU_HIP(hipSetDevice(device_));
        FSGPU_HIP(hipMemcpy(host_copy.data(), queries, host_copy.size() * 4, hipMemcpyDeviceToHost));
        queries = host_copy.data();
    }
    for (uint32_t i = 0; i < nq; ++i) {
        const float* q = queries + (size_t)i * dim_;
        uint32_t* rows = out_rows + (size_t)i * k;
        float* scores = out_scores + (size_t)i * k;
        if (bits == 0) FSGPU_TRY(search_hits(q, query_len, k, rows, scores, &out_counts[i]));
        else if (bits == 4) FSGPU_TRY(search_top_k_4bit_two_pass(q, query_len, k, multiplier, rows, scores, &out_counts[i]));
        else FSGPU_TRY(search_top_k_int8_two_pass(q, query_len, k, multiplier, rows, scores, &out_counts[i]));
    }
    if (fallbacks) *fallbacks = nq;
    return ok();
}

namespace {

struct HitsLayout {   // one device block per call; the three outputs adjacent at its end (fetch_batched_results: one copy up)
    size_t o_q, o_mrows, o_mscores, o_mcounts, o_wal, o_rows, o_scores, o_counts, total;
    HitsLayout(uint32_t nq, uint32_t dim, uint32_t k, uint32_t kw) {
        auto up = [](size_t v) { return (v + 255) / 256 * 256; };
        o_q = 0;
        o_mrows = up((size_t)nq * dim * 4);
        o_mscores = up(o_mrows + (size_t)nq * k * 4);
        o_mcounts = up(o_mscores + (size_t)nq * k * 4);
        o_wal = up(o_mcounts + (size_t)nq * 4);
        o_rows = up(o_wal + (size_t)nq * kw * 8);
        o_scores = up(o_rows + (size_t)nq * k * 4);
        o_counts = up(o_scores + (size_t)nq * k * 4);
        total = up(o_counts + (size_t)nq * 4);
    }
};

}  // namespace

// The resolve step's arguments over a call's block: main lists at their offsets, the WAL lists (kw > 0) and the class tables.
static ResolveHitsArgs resolve_args(unsigned char* base, const HitsLayout& lay, uint32_t nq, uint32_t k, uint32_t kw, uint64_t nrows,
                                    const uint64_t* live, const DeviceBuffer& main_class, const DeviceBuffer& wal_class,
                                    const DeviceBuffer& shadow) {
    ResolveHitsArgs ra;
    ra.main_rows = reinterpret_cast<const uint32_t*>(base + lay.o_mrows);
    ra.main_scores = reinterpret_cast<const float*>(base + lay.o_mscores);
    ra.main_counts = reinterpret_cast<const uint32_t*>(base + lay.o_mcounts);
    ra.wal_packed = kw ? reinterpret_cast<const u64*>(base + lay.o_wal) : nullptr;
    ra.live = reinterpret_cast<const u64*>(live);
    ra.shadowed = kw ? static_cast<const u64*>(shadow.ptr) : nullptr;
    ra.main_class = static_cast<const uint32_t*>(main_class.ptr);
    ra.wal_class = kw ? static_cast<const uint32_t*>(wal_class.ptr) : nullptr;
    ra.nq = nq;
    ra.k = k;
    ra.kw = kw;
    ra.nrows = (uint32_t)nrows;
    ra.out_rows = reinterpret_cast<uint32_t*>(base + lay.o_rows);
    ra.out_scores = reinterpret_cast<float*>(base + lay.o_scores);
    ra.out_counts = reinterpret_cast<uint32_t*>(base + lay.o_counts);
    return ra;
}

SearchError VectorIndex::search_hits_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t* out_rows,
                                             float* out_scores, uint32_t* out_counts, uint32_t* fallbacks, bool queries_on_device) {
    if (fallbacks) *fallbacks = 0;
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    FSGPU_TRY(ensure_query_dimension(query_len));
    if (nq == 0) return ok();
    if (any_search_parked())   // (this call reads the workspaces and the live bitmap of that search)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun batched search is outstanding on this index: end it first");
    const uint64_t W = wal_.size();
    const uint32_t kw = (uint32_t)std::min<uint64_t>(k, W);
    // what the device path does not cover, through the per-query call: no hits wanted, more than the resolve kernel's LDS lists hold,
    // rows beyond the packed row word, the catalog of a row-sharded index (its main rows come from the shards: topk_override), a
    // shard's row base, a dimension whose query does not fit the WAL kernel's LDS
    if (k == 0 || k > kHitsMaxK || nrows_ + W > 0xffffffffull || topk_override || catalog_only_ || row_base_ != 0 ||
        (kw && !wal_topk_supported(dim_, kw)))
        return hits_per_query(queries, nq, query_len, k, out_rows, out_scores, out_counts, fallbacks, queries_on_device, 0, 0);
    if (nrows_ == 0 && W == 0) {
        for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
        return ok();
    }
    FSGPU_TRY(ensure_hits_state());
    const HitsLayout lay(nq, dim_, k, kw);
    FSGPU_TRY(ws_hits_.reserve(lay.total));
    unsigned char* base = static_cast<unsigned char*>(ws_hits_.ptr);
    const float* q_dev = queries;
    if (!queries_on_device) {
        FSGPU_HIP(hipMemcpyAsync(base + lay.o_q, queries, (size_t)nq * dim_ * 4, hipMemcpyHostToDevice, stream_));
        q_dev = reinterpret_cast<const float*>(base + lay.o_q);
    }
    if (kw) {
        WalTopkArgs wa;
        wa.wal = static_cast<const float*>(hits_wal_.ptr);
        wa.queries = q_dev;
        wa.nq = nq;
        wa.W = (uint32_t)W;
        wa.dim = dim_;
        wa.kw = kw;
        wa.nrows = (uint32_t)nrows_;
        wa.hreduce = hreduce;
        wa.out_packed = reinterpret_cast<u64*>(base + lay.o_wal);
        wa.out_scores = nullptr;
        FSGPU_HIP(launch_wal_topk(wa, stream_));
    }
    uint32_t fb = 0;
    if (nrows_ > 0)
        FSGPU_TRY(search_top_k_batched_device(q_dev, nq, query_len, k, nullptr, reinterpret_cast<uint32_t*>(base + lay.o_mrows),
                                              reinterpret_cast<float*>(base + lay.o_mscores), reinterpret_cast<uint32_t*>(base + lay.o_mcounts),
                                              stream_, &fb));
    else
        FSGPU_HIP(hipMemsetAsync(base + lay.o_mcounts, 0, (size_t)nq * 4, stream_));
    FSGPU_HIP(launch_resolve_hits(resolve_args(base, lay, nq, k, kw, nrows_, live_dev_, hits_main_class_, hits_wal_class_, hits_shadow_), stream_));
    if (fallbacks) *fallbacks = fb;
    return fetch_batched_results(base, lay.o_rows, lay.o_scores, lay.o_counts, lay.total, nq, k, out_rows, out_scores, out_counts);
}

SearchError VectorIndex::search_hits_two_pass_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t multiplier,
                                                      int bits, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                                      uint32_t* fallbacks) {
    if (fallbacks) *fallbacks = 0;
    if (bits != 8 && bits != 4) return make_error(FSGPU_ERR_INVALID_CONFIG, "bits must be 8 or 4");
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    // where the per-query call takes the exact search (search.rs:579-585; quantized_two_pass), so does the batch
    if (k == 0 || nrows_ == 0 || !wal_.empty() || f32_)
        return search_hits_batched(queries, nq, query_len, k, out_rows, out_scores, out_counts, fallbacks);
    FSGPU_TRY(ensure_query_dimension(query_len));
    if (nq == 0) return ok();
    if (any_search_parked())
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun batched search is outstanding on this index: end it first");
    if (k > kHitsMaxK || nrows_ > 0xffffffffull || topk_override || catalog_only_ || row_base_ != 0)   // (as in search_hits_batched)
        return hits_per_query(queries, nq, query_len, k, out_rows, out_scores, out_counts, fallbacks, false, multiplier, bits);
    FSGPU_TRY(ensure_hits_state());
    const HitsLayout lay(nq, dim_, k, 0);
    FSGPU_TRY(ws_hits_.reserve(lay.total));
    unsigned char* base = static_cast<unsigned char*>(ws_hits_.ptr);
    FSGPU_HIP(hipMemcpyAsync(base + lay.o_q, queries, (size_t)nq * dim_ * 4, hipMemcpyHostToDevice, stream_));
    uint32_t fb = 0;
    // the row-level batched two-pass (no doc ids at that level); a query it answers per query arrives deduplicated already, and
    // the dedup of a deduplicated list changes nothing
    FSGPU_TRY(search_top_k_int8_batched_device(reinterpret_cast<const float*>(base + lay.o_q), nq, query_len, k, multiplier,
                                               reinterpret_cast<uint32_t*>(base + lay.o_mrows), reinterpret_cast<float*>(base + lay.o_mscores),
                                               reinterpret_cast<uint32_t*>(base + lay.o_mcounts), stream_, &fb, bits));
    FSGPU_HIP(launch_resolve_hits(resolve_args(base, lay, nq, k, 0, nrows_, live_dev_, hits_main_class_, hits_wal_class_, hits_shadow_), stream_));
    if (fallbacks) *fallbacks = fb;
    return fetch_batched_results(base, lay.o_rows, lay.o_scores, lay.o_counts, lay.total, nq, k, out_rows, out_scores, out_counts);
}

SearchError VectorIndex::lab_wal_scores(const float* queries, uint32_t nq, float* out) {
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    const size_t W = wal_.size();
    if (nq == 0 || W == 0) return ok();
    if (nrows_ + W > 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "too many rows for the device path");
    FSGPU_TRY(ensure_hits_state());
    const size_t qbytes = ((size_t)nq * dim_ * 4 + 255) / 256 * 256, obytes = (size_t)nq * W * 4;
    FSGPU_TRY(ws_hits_.reserve(qbytes + obytes));
    unsigned char* base = static_cast<unsigned char*>(ws_hits_.ptr);
    FSGPU_HIP(hipMemcpyAsync(base, queries, (size_t)nq * dim_ * 4, hipMemcpyHostToDevice, stream_));
    WalTopkArgs wa;
    wa.wal = static_cast<const float*>(hits_wal_.ptr);
    wa.queries = reinterpret_cast<const float*>(base);
    wa.nq = nq;
    wa.W = (uint32_t)W;
    wa.dim = dim_;
    wa.kw = 1;
    wa.nrows = (uint32_t)nrows_;
    wa.hreduce = hreduce;
    wa.out_packed = nullptr;
    wa.out_scores = reinterpret_cast<float*>(base + qbytes);
    FSGPU_HIP(launch_wal_topk(wa, stream_));
    FSGPU_HIP(hipMemcpyAsync(out, base + qbytes, obytes, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    return ok();
}

}  // namespace fsgpu

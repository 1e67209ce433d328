// vector_index_compact.cpp — the calls that let a long-lived index absorb its writes: append_batch, compact, vacuum, needs_*.
//
// Restated from crates/frankensearch-index/src/lib.rs:
//   append_batch_impl   :2569-2720   validate all, last-wins dedup, supersede resident copies, tombstone the first live main row
//   needs_compaction    :2270-2292   needs_vacuum :174, 2464-2475
//   compact             :2734-2854   live main rows + WAL entries, stable sort by (hash, doc id), adjacent duplicates collapse to the last
//   vacuum              :2485-2521   live main rows in order, WAL and generation kept
//   rewrite_index       :2871-3094   header | 16-byte records | strings | pad to 64 | slab; main rows raw, WAL rows encoded; flags cleared
//   next_generation     :6156
// The reference rewrites a file and opens it again.  Here the slab lives in device memory, so the vector pass is a device-to-device
// segmented copy (compact_kernels.hip) into a fresh allocation, the record tables are rebuilt on the host, and the file — when the
// caller names one — is written from the result.  Nothing of the index changes until all of that has succeeded.
#include <unistd.h>

#include <chrono>
#include <cmath>
#include <cstdio>
#include <numeric>
#include <unordered_map>

#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

namespace {

struct DocKey {
    uint64_t hash;
    const char* id;
    uint32_t len;
};
// (doc_id_hash, doc_id) as the writer and compact() order records: lib.rs:3753-3762, 2788-2793 (str::cmp is bytewise)
int cmp_key(const DocKey& a, const DocKey& b) {
    if (a.hash != b.hash) return a.hash < b.hash ? -1 : 1;
    const int c = std::memcmp(a.id, b.id, std::min(a.len, b.len));
    if (c != 0) return c;
    return a.len == b.len ? 0 : (a.len < b.len ? -1 : 1);
}

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

uint8_t next_generation(uint8_t g) { return g == 255 ? 1 : (uint8_t)(g + 1); }   // lib.rs:6156: 0 stays "never compacted"

}  // namespace

uint64_t VectorIndex::tombstone_count() const {
    if (live_host_.empty()) return 0;
    uint64_t live = 0;
    const size_t words = (size_t)((nrows_ + 63) / 64);
    for (size_t w = 0; w < words; ++w) {
        uint64_t v = live_host_[w];
        if (w + 1 == words && (nrows_ & 63)) v &= (1ull << (nrows_ & 63)) - 1ull;
        live += (uint64_t)__builtin_popcountll(v);
    }
    return nrows_ - live;
}

SearchError VectorIndex::fetch_live_host() {
    if (!live_host_.empty() || !live_dev_ || nrows_ == 0 || catalog_only_) return ok();
    // an adopted device slab (init_device) came with a device bitmap only: the plan is made on the host
    FSGPU_HIP(hipSetDevice(device_));
    std::vector<uint64_t> words((size_t)((nrows_ + 63) / 64));
    FSGPU_HIP(hipMemcpy(words.data(), live_dev_, words.size() * 8, hipMemcpyDeviceToHost));
    live_host_.swap(words);
    return ok();
}

bool VectorIndex::needs_compaction(uint64_t threshold, double ratio) const {
    if (wal_.empty()) return false;
    if (wal_.size() >= threshold) return true;
    if (nrows_ > 0) {
        const double r = (double)wal_.size() / (double)nrows_;
        if (r >= (std::isfinite(ratio) ? ratio : 0.10)) return true;   // a NaN ratio would switch the rule off: the default instead
    }
    return false;
}

SearchError VectorIndex::wal_append_batch(uint32_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors,
                                          uint32_t vector_len) {
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    if (any_search_parked())   // (its kernels read the live bitmap this call would rewrite)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun batched search is outstanding on this index: end it first");
    if (n == 0) return ok();
    if (!doc_ids || !vectors) return make_error(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    FSGPU_TRY(fetch_live_host());
    // every entry is validated before anything changes (lib.rs:2575-2602)
    if (vector_len != dim_)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "expected " + std::to_string(dim_) + ", found " + std::to_string(vector_len));
    std::vector<uint32_t> lens(n);
    for (uint32_t e = 0; e < n; ++e) {
        if (!doc_ids[e]) return make_error(FSGPU_ERR_NULL_ARGUMENT, "doc id is null");
        const float* v = vectors + (size_t)e * dim_;
        float norm_sq = 0.f;
        for (uint32_t i = 0; i < dim_; ++i) {
            if (!std::isfinite(v[i])) return make_error(FSGPU_ERR_INVALID_CONFIG, "all embedding values must be finite");
            const float p = v[i] * v[i];
            norm_sq = norm_sq + p;
        }
        if (!(norm_sq > 0.0f) || !std::isfinite(norm_sq))
            return make_error(FSGPU_ERR_INVALID_CONFIG, "embedding norm must be non-zero and finite");
        const size_t len = doc_id_lens ? doc_id_lens[e] : std::strlen(doc_ids[e]);
        if (len > 0xffffu) return make_error(FSGPU_ERR_INVALID_CONFIG, "doc_id byte length must fit in u16");
        lens[e] = (uint32_t)len;
    }
    // dedup within the batch, last wins, order of the survivors preserved (lib.rs:2604-2615)
    std::unordered_map<std::string, uint32_t> last;
    for (uint32_t e = 0; e < n; ++e) last[std::string(doc_ids[e], lens[e])] = e;
    // the tombstones first, on a copy: the one upload is the only step that can fail, and it comes before anything else changes
    std::vector<uint64_t> live = live_host_;
    bool changed = false;
    for (uint32_t e = 0; e < n; ++e) {
        if (last[std::string(doc_ids[e], lens[e])] != e) continue;
        // the first live main row with this doc id, so that it cannot take a top-k slot (lib.rs:2667-2711)
        const uint64_t h = fnv1a(doc_ids[e], lens[e]);
        auto lo = std::lower_bound(doc_hashes_.begin(), doc_hashes_.end(), h);
        for (auto it = lo; it != doc_hashes_.end() && *it == h; ++it) {
            const size_t r = (size_t)(it - doc_hashes_.begin());
            const size_t dl = (size_t)(doc_offsets_[r + 1] - doc_offsets_[r]);
            if (dl != lens[e] || std::memcmp(doc_blob_.data() + doc_offsets_[r], doc_ids[e], dl) != 0) continue;
            if (live.empty()) live.assign((size_t)((nrows_ + 63) / 64), ~0ull);
            if ((live[r >> 6] >> (r & 63)) & 1ull) {
                live[r >> 6] &= ~(1ull << (r & 63));
                changed = true;
                break;
            }
        }
    }
    if (changed) FSGPU_TRY(set_live_bitmap(live.data()));   // ONE upload per batch
    // supersede older resident copies (lib.rs:2641-2647), then admit the new entries
    wal_.erase(std::remove_if(wal_.begin(), wal_.end(), [&](const WalEntry& w) { return last.count(w.doc_id) != 0; }), wal_.end());
    for (uint32_t e = 0; e < n; ++e) {
        std::string id(doc_ids[e], lens[e]);
        if (last[id] != e) continue;
        const float* v = vectors + (size_t)e * dim_;
        wal_.push_back(WalEntry{std::move(id), std::vector<float>(v, v + dim_)});
    }
    invalidate_hits_state(false);   // the WAL mirror, its classes and the shadowed rows of search_hits_batched
    return ok();
}

// What rules a rewrite out before it starts.
SearchError VectorIndex::rewrite_refusal() const {
    if (catalog_only_)
        return make_error(FSGPU_ERR_INVALID_CONFIG,
                          "compact / vacuum of a row-sharded index is not supported: the rows would have to be re-sharded");
    if (any_search_parked())   // (its kernels read the slab this call would replace)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun batched search is outstanding on this index: end it first");
    if (lone_.kind != kLoneNone) return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun lone search is outstanding on this index: end it first");
    if (row_stride_ && row_stride_ != dim_ * (f32_ ? 4u : 2u))
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a strided view of another index's slab cannot be rewritten");
    return ok();
}

SearchError VectorIndex::compact(const char* path, CompactionStats* out) {
    const auto t0 = std::chrono::steady_clock::now();
    FSGPU_TRY(rewrite_refusal());
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    CompactionStats st;
    st.main_records_before = nrows_;
    if (wal_.empty()) {   // no-op, tombstones stay (lib.rs:2740-2747)
        st.total_records_after = nrows_;
        if (out) *out = st;
        return ok();
    }
    st.wal_records = wal_.size();
    last_rewrite = RewriteTimes{};
    // The plan.  The record table is sorted already, so the reference's sort of N + W keys is a MERGE of the live main rows with
    // the W sorted WAL entries; ties put the main row first (the sort is stable and main rows are collected first), and adjacent
    // equal keys collapse to the last — WAL beats main, of two live main duplicates the higher row wins.
    const size_t W = wal_.size();
    std::vector<uint64_t> wal_hash(W);
    for (size_t w = 0; w < W; ++w) wal_hash[w] = fnv1a(wal_[w].doc_id.data(), wal_[w].doc_id.size());
    auto key_of = [&](uint64_t src) {
        if (src & kWalSource) {
            const size_t w = (size_t)(src & ~kWalSource);
            return DocKey{wal_hash[w], wal_[w].doc_id.data(), (uint32_t)wal_[w].doc_id.size()};
        }
        return DocKey{doc_hashes_[src], doc_blob_.data() + doc_offsets_[src], (uint32_t)(doc_offsets_[src + 1] - doc_offsets_[src])};
    };
    std::vector<uint64_t> wal_order(W);
    std::iota(wal_order.begin(), wal_order.end(), 0ull);
    std::stable_sort(wal_order.begin(), wal_order.end(),
                     [&](uint64_t a, uint64_t b) { return cmp_key(key_of(kWalSource | a), key_of(kWalSource | b)) < 0; });
    std::vector<uint64_t> sources;
    sources.reserve((size_t)nrows_ + W);
    auto emit = [&](uint64_t src) {
        if (!sources.empty() && cmp_key(key_of(sources.back()), key_of(src)) == 0) sources.back() = src;
        else sources.push_back(src);
    };
    bool sorted = true;
    size_t j = 0;
    int64_t prev = -1;
    for (uint64_t r = 0; r < nrows_ && sorted; ++r) {
        if (row_tombstoned(r)) continue;
        const DocKey k = key_of(r);
        if (prev >= 0 && cmp_key(key_of((uint64_t)prev), k) > 0) sorted = false;   // (not written by VectorIndexWriter)
        prev = (int64_t)r;
        while (j < W && cmp_key(key_of(kWalSource | wal_order[j]), k) < 0) emit(kWalSource | wal_order[j++]);
        emit(r);
    }
    while (sorted && j < W) emit(kWalSource | wal_order[j++]);
    if (!sorted) {   // a record table out of order: the reference's sort as it stands
        std::vector<uint64_t> all;
        all.reserve((size_t)nrows_ + W);
        for (uint64_t r = 0; r < nrows_; ++r)
            if (!row_tombstoned(r)) all.push_back(r);
        for (size_t w = 0; w < W; ++w) all.push_back(kWalSource | w);
        std::stable_sort(all.begin(), all.end(), [&](uint64_t a, uint64_t b) { return cmp_key(key_of(a), key_of(b)) < 0; });
        sources.clear();
        for (uint64_t s : all) emit(s);
    }
    last_rewrite.plan_ms = ms_since(t0);
    FSGPU_TRY(rewrite(sources, next_generation(compaction_gen_), true, path));
    st.total_records_after = nrows_;
    st.elapsed_ms = ms_since(t0);
    if (out) *out = st;
    return ok();
}

SearchError VectorIndex::vacuum(const char* path, VacuumStats* out) {
    const auto t0 = std::chrono::steady_clock::now();
    FSGPU_TRY(rewrite_refusal());
    FSGPU_TRY(fetch_live_host());
    VacuumStats st;
    st.records_before = st.records_after = nrows_;
    const uint64_t tombstones = tombstone_count();
    if (nrows_ == 0 || tombstones == 0) {   // lib.rs:2492-2500
        if (out) *out = st;
        return ok();
    }
    if (path && doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "an FSVI image needs a doc-id table: this index has none");
    last_rewrite = RewriteTimes{};
    const uint64_t row_bytes = (uint64_t)dim_ * (f32_ ? 4 : 2);
    const uint64_t bytes_before = from_fsvi_ ? fsvi_image_bytes(nrows_, doc_blob_.size()) : nrows_ * row_bytes;
    std::vector<uint64_t> sources;
    sources.reserve((size_t)(nrows_ - tombstones));
    for (uint64_t r = 0; r < nrows_; ++r)
        if (!row_tombstoned(r)) sources.push_back(r);
    last_rewrite.plan_ms = ms_since(t0);
    FSGPU_TRY(rewrite(sources, compaction_gen_, false, path));
    const uint64_t bytes_after = from_fsvi_ ? fsvi_image_bytes(nrows_, doc_blob_.size()) : nrows_ * row_bytes;
    st.records_after = nrows_;
    st.tombstones_removed = st.records_before - st.records_after;
    st.bytes_reclaimed = bytes_before > bytes_after ? bytes_before - bytes_after : 0;
    st.elapsed_ms = ms_since(t0);
    if (out) *out = st;
    return ok();
}

// Length of the FSVI v1 image of `rows` records whose doc ids take strings_len bytes (rewrite_index's layout, lib.rs:2925-2952)
uint64_t VectorIndex::fsvi_image_bytes(uint64_t rows, uint64_t strings_len) const {
    const uint64_t header_len = 4 + 2 + 2 + embedder_id_.size() + 2 + embedder_revision_.size() + 4 + 1 + 3 + 8 + 8 + 4;
    const uint64_t pre = header_len + rows * 16 + strings_len;
    return (pre + 63) / 64 * 64 + rows * dim_ * (f32_ ? 4 : 2);
}

SearchError VectorIndex::rewrite(const std::vector<uint64_t>& sources, uint8_t new_gen, bool clear_wal, const char* path) {
    FSGPU_HIP(hipSetDevice(device_));
    const uint64_t n_new = sources.size();
    if (n_new + row_base_ >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row ids must fit in u32 (VectorHit.index)");
    const uint64_t row_bytes = (uint64_t)dim_ * (f32_ ? 4 : 2);
    const bool tables = !doc_offsets_.empty();
    auto t = std::chrono::steady_clock::now();

    // ---- runs: maximal stretches of consecutive rows of one source; the surviving WAL rows form a block in output order ----
    std::vector<CompactRun> runs;
    std::vector<uint32_t> wal_rows;   // WAL indexes in output order
    std::vector<RewriteRun> source_runs;   // the same runs in rows, for rewrite_sources
    {
        uint64_t expect = ~0ull;   // the source that would extend the current run
        for (uint64_t i = 0; i < n_new; ++i) {
            const uint64_t s = sources[(size_t)i];
            uint64_t pos;
            if (s & kWalSource) {
                pos = kWalSource | wal_rows.size();
                wal_rows.push_back((uint32_t)(s & ~kWalSource));
            } else {
                pos = s;
            }
            if (pos != expect) {
                runs.push_back(CompactRun{(pos & kWalSource) | ((pos & ~kWalSource) * row_bytes), i * row_bytes});
                source_runs.push_back(RewriteRun{i, (s & kWalSource) ? kWalSource : s});
            }
            expect = pos + 1;
        }
        runs.push_back(CompactRun{0, n_new * row_bytes});   // the end marker
        source_runs.push_back(RewriteRun{n_new, 0});
    }
    const uint64_t nruns = runs.size() - 1;
    last_rewrite.runs = nruns;
    last_rewrite.dst_bytes = n_new * row_bytes;

    // ---- everything is allocated before anything is touched ----
    DeviceBuffer fresh, runs_dev, wal_f32, wal_enc, wal_perm;
    auto release_all = [&]() {
        for (DeviceBuffer* b : {&fresh, &runs_dev, &wal_f32, &wal_enc, &wal_perm}) b->release();
    };
    SearchError e = fresh.reserve((size_t)(n_new * row_bytes));
    if (e.ok()) e = runs_dev.reserve(runs.size() * sizeof(CompactRun));
    const size_t nw = wal_rows.size();
    if (e.ok() && nw) e = wal_f32.reserve(nw * (size_t)dim_ * 4);
    if (e.ok() && nw && !f32_) e = wal_enc.reserve(nw * (size_t)row_bytes);
    if (e.ok() && nw && !f32_) e = wal_perm.reserve(nw * 4);
    if (!e.ok()) {
        release_all();
        return e;
    }
    auto fail_hip = [&](hipError_t he, const char* what) {
        (void)hipStreamSynchronize(stream_);
        release_all();
        return hip_fail(he, what);
    };
    hipError_t he = hipMemcpyAsync(runs_dev.ptr, runs.data(), runs.size() * sizeof(CompactRun), hipMemcpyHostToDevice, stream_);
    if (he != hipSuccess) return fail_hip(he, "upload of the runs");
    std::vector<float> wal_block;
    if (nw) {
        // WAL rows: raw little-endian f32 on an F32 slab; on an F16 slab through the device's round-to-nearest-even encoder, the one
        // the FSVI writer uses (lib.rs:3015-3021, 3035-3041)
        wal_block.resize(nw * (size_t)dim_);
        for (size_t i = 0; i < nw; ++i) std::memcpy(&wal_block[i * dim_], wal_[wal_rows[i]].embedding.data(), (size_t)dim_ * 4);
        he = hipMemcpyAsync(wal_f32.ptr, wal_block.data(), wal_block.size() * 4, hipMemcpyHostToDevice, stream_);
        if (he == hipSuccess && !f32_) {
            std::vector<uint32_t> identity(nw);
            std::iota(identity.begin(), identity.end(), 0u);
            he = hipMemcpy(wal_perm.ptr, identity.data(), nw * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = launch_encode_rows_f16(static_cast<const float*>(wal_f32.ptr), static_cast<const uint32_t*>(wal_perm.ptr), nw, dim_,
                                            static_cast<unsigned short*>(wal_enc.ptr), stream_);
        }
        if (he != hipSuccess) return fail_hip(he, "encoding of the WAL rows");
    }
    he = hipStreamSynchronize(stream_);
    if (he != hipSuccess) return fail_hip(he, "hipStreamSynchronize");
    last_rewrite.plan_ms += ms_since(t);

    // ---- the vector pass ----
    t = std::chrono::steady_clock::now();
    CompactArgs a;
    a.slab = static_cast<const unsigned char*>(slab_dev_);
    a.wal = static_cast<const unsigned char*>(f32_ ? wal_f32.ptr : wal_enc.ptr);
    a.out = static_cast<unsigned char*>(fresh.ptr);
    a.runs = static_cast<const CompactRun*>(runs_dev.ptr);
    a.nruns = nruns;
    const uint64_t launch_bytes = (uint64_t)(compact_launch_rows ? compact_launch_rows : kCompactLaunchRows) * row_bytes;
    for (uint64_t b0 = 0; b0 < n_new * row_bytes; b0 += launch_bytes) {
        a.dst_begin = b0;
        a.dst_end = std::min(b0 + launch_bytes, n_new * row_bytes);
        he = launch_compact_runs(a, compact_nt_stores, stream_);
        if (he != hipSuccess) return fail_hip(he, "launch_compact_runs");
        ++last_rewrite.launches;
    }
    he = hipStreamSynchronize(stream_);
    if (he != hipSuccess) return fail_hip(he, "hipStreamSynchronize");
    last_rewrite.kernel_ms = ms_since(t);

    // ---- the record tables of the new rows ----
    t = std::chrono::steady_clock::now();
    std::vector<uint64_t> hashes, offsets;
    std::string blob;
    if (tables) {
        hashes.resize((size_t)n_new);
        offsets.resize((size_t)n_new + 1);
        blob.reserve(doc_blob_.size());
        for (uint64_t i = 0; i < n_new; ++i) {
            const uint64_t s = sources[(size_t)i];
            offsets[(size_t)i] = blob.size();
            if (s & kWalSource) {
                const std::string& id = wal_[(size_t)(s & ~kWalSource)].doc_id;
                hashes[(size_t)i] = fnv1a(id.data(), id.size());
                blob.append(id);
            } else {
                hashes[(size_t)i] = doc_hashes_[(size_t)s];
                blob.append(doc_blob_, (size_t)doc_offsets_[(size_t)s], (size_t)(doc_offsets_[(size_t)s + 1] - doc_offsets_[(size_t)s]));
            }
        }
        offsets[(size_t)n_new] = blob.size();
        if (blob.size() > 0xffffffffull) {
            release_all();
            return make_error(FSGPU_ERR_INVALID_CONFIG, "string table offset exceeds u32");
        }
    }
    last_rewrite.tables_ms = ms_since(t);

    // ---- the file, when asked for: a temporary name beside the target, renamed over it (lib.rs:2961-3053) ----
    if (path) {
        t = std::chrono::steady_clock::now();
        const uint64_t image_bytes = fsvi_image_bytes(n_new, blob.size());
        const uint64_t vectors_offset = image_bytes - n_new * row_bytes;
        std::vector<uint8_t> head((size_t)vectors_offset, 0);
        auto put = [&](size_t at, uint64_t v, int bytes) {
            for (int b = 0; b < bytes; ++b) head[at + b] = (uint8_t)(v >> (8 * b));
        };
        size_t c = 0;
        std::memcpy(head.data(), "FSVI", 4);
        c += 4;
        put(c, 1, 2);
        c += 2;
        for (const std::string* sfield : {&embedder_id_, &embedder_revision_}) {
            put(c, sfield->size(), 2);
            c += 2;
            std::memcpy(head.data() + c, sfield->data(), sfield->size());
            c += sfield->size();
        }
        put(c, dim_, 4);
        c += 4;
        head[c++] = f32_ ? 0 : 1;
        head[c++] = new_gen;
        put(c, publication_nonce_, 2);
        c += 2;
        put(c, n_new, 8);
        c += 8;
        put(c, vectors_offset, 8);
        c += 8;
        put(c, crc32_ieee(head.data(), c), 4);
        c += 4;
        for (uint64_t i = 0; i < n_new; ++i) {
            put(c + (size_t)i * 16, hashes[(size_t)i], 8);
            put(c + (size_t)i * 16 + 8, offsets[(size_t)i], 4);
            put(c + (size_t)i * 16 + 12, offsets[(size_t)i + 1] - offsets[(size_t)i], 2);
        }
        std::memcpy(head.data() + c + (size_t)n_new * 16, blob.data(), blob.size());
        const std::string tmp = std::string(path) + ".tmp";
        SearchError fe = ok();
        FILE* f = std::fopen(tmp.c_str(), "wb");
        if (!f) fe = make_error(FSGPU_ERR_IO, "cannot create " + tmp);
        if (fe.ok() && std::fwrite(head.data(), 1, head.size(), f) != head.size()) fe = make_error(FSGPU_ERR_IO, "short write to " + tmp);
        std::vector<uint8_t> chunk;
        const uint64_t kChunk = 64ull << 20;
        for (uint64_t b0 = 0; fe.ok() && b0 < n_new * row_bytes; b0 += kChunk) {
            const size_t nb = (size_t)std::min(kChunk, n_new * row_bytes - b0);
            chunk.resize(nb);
            he = hipMemcpy(chunk.data(), static_cast<const unsigned char*>(fresh.ptr) + b0, nb, hipMemcpyDeviceToHost);
            if (he != hipSuccess) fe = hip_fail(he, "download of the new slab");
            else if (std::fwrite(chunk.data(), 1, nb, f) != nb) fe = make_error(FSGPU_ERR_IO, "short write to " + tmp);
        }
        if (f) {
            if (fe.ok() && (std::fflush(f) != 0 || fsync(fileno(f)) != 0)) fe = make_error(FSGPU_ERR_IO, "cannot flush " + tmp);
            std::fclose(f);
        }
        if (fe.ok() && std::rename(tmp.c_str(), path) != 0) fe = make_error(FSGPU_ERR_IO, std::string("cannot rename over ") + path);
        if (!fe.ok()) {
            if (f) std::remove(tmp.c_str());
            release_all();
            return fe;
        }
        last_rewrite.file_ms = ms_since(t);
    }

    // ---- commit: from here on nothing fails ----
    (void)hipDeviceSynchronize();   // (no search may be in flight on this handle; whatever a lane left queued has drained)
    if (owns_slab_) slab_own_.release();   // an adopted slab stays its owner's: it is no longer referenced from here on
    slab_own_ = fresh;
    fresh = DeviceBuffer{};
    slab_dev_ = slab_own_.ptr;
    owns_slab_ = true;
    const uint64_t old_rows = nrows_;
    nrows_ = n_new;
    live_host_.clear();   // all flags cleared (lib.rs:2919)
    live_dev_ = nullptr;
    live_own_.release();
    if (tables) {
        doc_hashes_.swap(hashes);
        doc_offsets_.swap(offsets);
        doc_blob_.swap(blob);
    }
    if (clear_wal) wal_.clear();
    compaction_gen_ = new_gen;
    ++generation_;
    rewrite_old_rows_ = old_rows;
    rewrite_generation_ = generation_;
    rewrite_runs_.swap(source_runs);
    release_all();
    t = std::chrono::steady_clock::now();
    drop_derived_state();
    // lone-query latency does not depend on history.  (An error from here on leaves the NEW index, whole and searchable: only the
    // copies are missing, and the first search that wants them builds them.)
    SearchError re = ok();
    if (int8_latency && int8_latency_build_now) re = prepare_int8_latency();
    last_rewrite.rebuild_ms = ms_since(t);
    return re;
}

SearchError VectorIndex::rewrite_sources(uint32_t* out_new_to_old, uint64_t* generation_before, uint64_t* generation_after,
                                         uint64_t* old_record_count) const {
    if (rewrite_generation_ == 0 || rewrite_runs_.empty())
        return make_error(FSGPU_ERR_INVALID_CONFIG, "no compaction or vacuum has rewritten the slab on this handle");
    if (rewrite_runs_.back().first != nrows_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the kept runs do not describe this slab");
    if (nrows_ && !out_new_to_old) return make_error(FSGPU_ERR_NULL_ARGUMENT, "out_new_to_old is null");
    for (size_t r = 0; r + 1 < rewrite_runs_.size(); ++r) {
        const RewriteRun& run = rewrite_runs_[r];
        const uint64_t end = rewrite_runs_[r + 1].first;
        for (uint64_t i = run.first; i < end; ++i)
            out_new_to_old[i] = (run.src & kWalSource) ? kKnnPadRow : (uint32_t)(run.src + (i - run.first));
    }
    if (generation_before) *generation_before = rewrite_generation_ - 1;
    if (generation_after) *generation_after = rewrite_generation_;
    if (old_record_count) *old_record_count = rewrite_old_rows_;
    return ok();
}

SearchError VectorIndex::lab_attach_synthetic_doc_ids() {
    if (!doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "the index has a doc-id table already");
    if (catalog_only_ || row_base_ != 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "a whole, unsharded index only");
    constexpr size_t kLen = 13;   // "doc-" + 9 digits
    std::vector<std::pair<uint64_t, uint64_t>> keyed((size_t)nrows_);   // (hash, number): equal lengths, so ties order by number
    char id[kLen + 1];
    for (uint64_t i = 0; i < nrows_; ++i) {
        std::snprintf(id, sizeof id, "doc-%09llu", (unsigned long long)i);
        keyed[(size_t)i] = {fnv1a(id, kLen), i};
    }
    std::sort(keyed.begin(), keyed.end());
    doc_hashes_.resize((size_t)nrows_);
    doc_offsets_.resize((size_t)nrows_ + 1);
    doc_blob_.resize((size_t)nrows_ * kLen);
    for (uint64_t r = 0; r < nrows_; ++r) {
        std::snprintf(id, sizeof id, "doc-%09llu", (unsigned long long)keyed[(size_t)r].second);
        doc_hashes_[(size_t)r] = keyed[(size_t)r].first;
        doc_offsets_[(size_t)r] = r * kLen;
        std::memcpy(&doc_blob_[(size_t)r * kLen], id, kLen);
    }
    doc_offsets_[(size_t)nrows_] = nrows_ * kLen;
    embedder_id_ = "bench";
    invalidate_hits_state(true);
    return ok();
}

// Everything derived from row ids or slab contents: the quantised copies, the measured statistics, the views and the lanes.
void VectorIndex::drop_derived_state() {
    for (DeviceBuffer* b : {&i8_slab_, &n4_slab_, &n4u_slab_, &i8_stats_, &i8f_slab_, &i8f_max_, &i8f_stats_, &mf_max_norm_}) b->release();
    if (!quant_max_ready_) i8_max_.release();   // (a corpus-wide max-abs handed in by a sharded parent is not this slab's to drop)
    i8_ready_ = n4_ready_ = n4u_ready_ = i8_stats_ready_ = false;
    i8f_decided_ = i8f_rot_ = i8f_ready_ = false;
    mf_norm_ready_ = false;
    i8f_disabled_ = false;
    i8f_strikes_ = 0;
    i8f_sample_boost_ = 1;
    cert_skip_ = cert_backoff_ = tp_skip_ = tp_backoff_ = 0;
    mf_pass_parity_ = 0;
    views_.clear();
    replicas_.clear();
    invalidate_hits_state(true);   // search_hits_batched: the classes number rows of the old record table
}

}  // namespace fsgpu

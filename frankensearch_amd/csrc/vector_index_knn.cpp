// vector_index_knn.cpp — the exact k-NN graph over a VectorIndex's main slab (include/fsgpu.h, fsgpu_index_build_knn_graph).
//
// knn(i, m) is defined by the index's own row-level search, so the build is a driver around the batched search and scans nothing
// itself: per step up to kKnnChunk live sources are staged from the slab into an f32 query block (knn_stage_rows_kernel), searched
// with k = m + 1 through search_top_k_batched_device_begin / _end, and their hits turned into lists (knn_emit_kernel).  Two steps
// are in flight: while the host ends step c - 1, emits it and copies its lists out, step c's search runs.  The emit and the copy to
// the pinned block go on a stream of their own behind an event recorded after the step's begin — or, when end() reported late
// answers (hits written by work enqueued in end), behind an event recorded after those.
#include <vector>

#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

namespace {

struct KnnStep {   // one step in flight: offsets into its device block and its pinned block
    unsigned char* dev = nullptr;
    unsigned char* pin = nullptr;
    hipEvent_t searched = nullptr;
    int32_t ticket = -1;
    uint32_t n = 0;
    std::vector<uint32_t> src;   // local source rows, as staged
};

struct KnnScratch {   // what a build owns besides the index's workspaces: released on every return path
    hipStream_t emit_stream = nullptr;
    void* pinned = nullptr;
    KnnStep step[2];
    ~KnnScratch() {
        for (KnnStep& s : step)
            if (s.searched) (void)hipEventDestroy(s.searched);
        if (emit_stream) (void)hipStreamDestroy(emit_stream);
        if (pinned) (void)hipHostFree(pinned);
    }
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

SearchError VectorIndex::knn_stage_rows_host(const uint32_t* src_local, uint32_t n, float* out) {
    if (catalog_only_ || (!slab_dev_ && nrows_ > 0)) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (n == 0) return ok();
    FSGPU_HIP(hipSetDevice(device_));
    const size_t q_bytes = (size_t)n * dim_ * 4, o_src = align256(q_bytes), o_list = align256(o_src + (size_t)n * 4);
    FSGPU_TRY(ws_knn_[0].reserve(o_list + (size_t)n * 4));
    unsigned char* dev = static_cast<unsigned char*>(ws_knn_[0].ptr);
    FSGPU_HIP(hipMemcpyAsync(dev + o_list, src_local, (size_t)n * 4, hipMemcpyHostToDevice, stream_));
    KnnStageArgs a{};
    a.slab = slab_dev_;
    a.row_stride = row_stride_ ? row_stride_ : dim_ * (f32_ ? 4u : 2u);
    a.dim = dim_;
    a.slab_f32 = f32_ ? 1u : 0u;
    a.row_base = (uint32_t)row_base_;
    a.src_local = reinterpret_cast<const uint32_t*>(dev + o_list);
    a.n = n;
    a.queries = reinterpret_cast<float*>(dev);
    a.src_out = reinterpret_cast<uint32_t*>(dev + o_src);
    FSGPU_HIP(launch_knn_stage_rows(a, stream_));
    FSGPU_HIP(hipMemcpyAsync(out, dev, q_bytes, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    return ok();
}

SearchError VectorIndex::build_knn_graph(uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t* out_rows, float* out_sims) {
    last_knn_build = KnnBuildStats{};
    if (m < 1 || m > kKnnMaxM) return make_error(FSGPU_ERR_INVALID_CONFIG, "m must be 1 .. 63 (k = m + 1 stays inside the fused tiers)");
    if (first_row > nrows_ || n_rows > nrows_ - first_row)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "source rows " + std::to_string(first_row) + " .. " + std::to_string(first_row + n_rows) +
                                                        " lie past record_count " + std::to_string(nrows_));
    if (n_rows == 0) return ok();
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (tickets_taken() != 0 || lone_.kind != kLoneNone)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun search is outstanding on this index: end it first (the build takes both tickets)");
    FSGPU_TRY(fetch_live_host());

    const size_t list_bytes = (size_t)m * 4;
    uint64_t next = first_row;
    const uint64_t end = first_row + n_rows;
    // the next chunk's live sources; a tombstoned source costs no scan work: its list is padding, written here
    auto next_chunk = [&](std::vector<uint32_t>& src, uint32_t cap) {
        while (next < end && src.size() < cap) {
            if (row_tombstoned(next)) {
                const size_t at = (size_t)(next - first_row) * m;
                for (uint32_t x = 0; x < m; ++x) out_rows[at + x] = kKnnPadRow;
                if (out_sims)
                    for (uint32_t x = 0; x < m; ++x) out_sims[at + x] = 0.0f;
            } else {
                src.push_back((uint32_t)next);
            }
            ++next;
        }
        return next < end;
    };
    // the chunk's sources are ascending; where they are consecutive rows (no tombstone between them) the lists go in one copy
    auto sink = [&](const KnnStepLists& s) -> SearchError {
        uint32_t i = 0;
        while (i < s.n) {
            uint32_t j = i + 1;
            while (j < s.n && s.src[j] == s.src[j - 1] + 1) ++j;
            const size_t at = (size_t)(s.src[i] - first_row) * m;
            std::memcpy(out_rows + at, s.rows_host + (size_t)i * m, (size_t)(j - i) * list_bytes);
            if (out_sims) std::memcpy(out_sims + at, s.sims_host + (size_t)i * m, (size_t)(j - i) * list_bytes);
            i = j;
        }
        return ok();
    };
    return knn_search_steps((uint32_t)std::min<uint64_t>(kKnnChunk, n_rows), m, out_sims != nullptr, true, next_chunk, sink);
}

// The step loop of the build, over whatever sources next_chunk hands out (ascending local rows, up to cap per call; it returns
// whether more may follow).  A drained step's lists reach `sink` in the pinned block (lists_to_host) or still in the step's device
// block, on the emit stream, which is synchronised after the sink returns: the block is staged into again two steps later.
SearchError VectorIndex::knn_search_steps(uint32_t cap, uint32_t m, bool want_sims, bool lists_to_host, const KnnNextChunk& next_chunk,
                                          const KnnStepSink& sink) {
    if (cap == 0) return ok();
    FSGPU_HIP(hipSetDevice(device_));

    const uint32_t k = m + 1;
    // device block of a step: queries | global sources | hit rows | hit scores | counts | out rows, out sims (the step's n * m rows,
    // then its n * m sims directly behind them: ONE copy brings both up)
    const size_t o_src = align256((size_t)cap * dim_ * 4), o_hrows = align256(o_src + (size_t)cap * 4),
                 o_hscores = align256(o_hrows + (size_t)cap * k * 4), o_counts = align256(o_hscores + (size_t)cap * k * 4),
                 o_out = align256(o_counts + (size_t)cap * 4), dev_bytes = align256(o_out + 2 * (size_t)cap * m * 4);
    // pinned block of a step: local sources (read in place by the stage kernel) | out rows, out sims
    const size_t p_out = align256((size_t)cap * 4), pin_bytes = align256(p_out + 2 * (size_t)cap * m * 4);
    KnnScratch sc;
    FSGPU_HIP(hipStreamCreateWithFlags(&sc.emit_stream, hipStreamNonBlocking));
    FSGPU_HIP(hipHostMalloc(&sc.pinned, 2 * pin_bytes, hipHostMallocDefault));
    for (int s = 0; s < 2; ++s) {
        FSGPU_TRY(ws_knn_[s].reserve(dev_bytes));
        sc.step[s].dev = static_cast<unsigned char*>(ws_knn_[s].ptr);
        sc.step[s].pin = static_cast<unsigned char*>(sc.pinned) + (size_t)s * pin_bytes;
        FSGPU_HIP(hipEventCreateWithFlags(&sc.step[s].searched, hipEventDisableTiming));
        sc.step[s].src.reserve(cap);
    }
    const size_t list_bytes = (size_t)m * 4;

    // a failure in mid-build must leave no ticket behind: end what was begun (its verdicts are not needed) before returning
    auto abandon = [&](SearchError e) {
        for (KnnStep& s : sc.step)
            if (s.ticket >= 0) {
                (void)search_top_k_batched_device_end(s.ticket, nullptr, nullptr);
                s.ticket = -1;
            }
        (void)hipStreamSynchronize(stream_);
        (void)hipStreamSynchronize(sc.emit_stream);
        return e;
    };

    auto begin_step = [&](KnnStep& s) -> SearchError {
        std::memcpy(s.pin, s.src.data(), (size_t)s.n * 4);
        KnnStageArgs a{};
        a.slab = slab_dev_;
        a.row_stride = row_stride_ ? row_stride_ : dim_ * (f32_ ? 4u : 2u);
        a.dim = dim_;
        a.slab_f32 = f32_ ? 1u : 0u;
        a.row_base = (uint32_t)row_base_;
        a.src_local = reinterpret_cast<const uint32_t*>(s.pin);
        a.n = s.n;
        a.queries = reinterpret_cast<float*>(s.dev);
        a.src_out = reinterpret_cast<uint32_t*>(s.dev + o_src);
        FSGPU_HIP(launch_knn_stage_rows(a, stream_));
        FSGPU_TRY(search_top_k_batched_device_begin(reinterpret_cast<const float*>(s.dev), s.n, dim_, k, nullptr,
                                                    reinterpret_cast<uint32_t*>(s.dev + o_hrows), reinterpret_cast<float*>(s.dev + o_hscores),
                                                    reinterpret_cast<uint32_t*>(s.dev + o_counts), stream_, nullptr, &s.ticket));
        FSGPU_HIP(hipEventRecord(s.searched, stream_));
        return ok();
    };

    auto drain_step = [&](KnnStep& s) -> SearchError {
        uint32_t fb = 0, late = 0;
        const int32_t t = s.ticket;
        s.ticket = -1;
        FSGPU_TRY(search_top_k_batched_device_end(t, &fb, &late));
        last_knn_build.fallbacks += fb;
        last_knn_build.late_answers += late;
        // late answers were written by work end() enqueued on the search stream, behind `searched`: the lists wait for them
        if (late) FSGPU_HIP(hipEventRecord(s.searched, stream_));
        FSGPU_HIP(hipStreamWaitEvent(sc.emit_stream, s.searched, 0));
        KnnEmitArgs e{};
        e.hit_rows = reinterpret_cast<const uint32_t*>(s.dev + o_hrows);
        e.hit_scores = reinterpret_cast<const float*>(s.dev + o_hscores);
        e.hit_counts = reinterpret_cast<const uint32_t*>(s.dev + o_counts);
        e.src = reinterpret_cast<const uint32_t*>(s.dev + o_src);
        e.n = s.n;
        e.m = m;
        e.out_rows = reinterpret_cast<uint32_t*>(s.dev + o_out);
        e.out_sims = want_sims ? reinterpret_cast<float*>(s.dev + o_out + (size_t)s.n * list_bytes) : nullptr;
        FSGPU_HIP(launch_knn_emit(e, sc.emit_stream));
        KnnStepLists l{};
        l.src = s.src.data();
        l.n = s.n;
        l.src_dev = e.src;
        l.rows_dev = e.out_rows;
        l.sims_dev = e.out_sims;
        l.stream = sc.emit_stream;
        if (lists_to_host) {
            FSGPU_HIP(hipMemcpyAsync(s.pin + p_out, s.dev + o_out, (size_t)s.n * list_bytes * (want_sims ? 2 : 1), hipMemcpyDeviceToHost,
                                     sc.emit_stream));
            FSGPU_HIP(hipStreamSynchronize(sc.emit_stream));
            l.rows_host = reinterpret_cast<const uint32_t*>(s.pin + p_out);
            l.sims_host = want_sims ? reinterpret_cast<const float*>(s.pin + p_out + (size_t)s.n * list_bytes) : nullptr;
        }
        FSGPU_TRY(sink(l));
        if (!lists_to_host) FSGPU_HIP(hipStreamSynchronize(sc.emit_stream));
        last_knn_build.steps += 1;
        last_knn_build.sources += s.n;
        return ok();
    };

    uint64_t c = 0;
    bool more = true;
    while (true) {
        KnnStep& cur = sc.step[c & 1];
        cur.n = 0;
        cur.src.clear();
        if (more) {
            more = next_chunk(cur.src, cap);
            cur.n = (uint32_t)cur.src.size();
            if (cur.n) {
                const SearchError e = begin_step(cur);
                if (!e.ok()) return abandon(e);
            }
        }
        if (c >= 1) {
            KnnStep& prev = sc.step[(c - 1) & 1];
            if (prev.ticket >= 0) {
                const SearchError e = drain_step(prev);
                if (!e.ok()) return abandon(e);
            }
        }
        if (cur.n == 0) break;   // nothing was begun in this round and the round before is drained
        ++c;
    }
    return ok();
}

}  // namespace fsgpu

// vector_index_knn_update.cpp — carrying the exact k-NN table of a VectorIndex across a compaction, a vacuum or deletes
// (include/fsgpu.h, fsgpu_index_update_knn_graph).
//
// The old table and the map new row -> old row go down once.  The device builds the inverse map, classifies every current row
// (dead / added / kept-clean / kept-dirty) and writes the kept-clean rows' remapped lists into a working table [n, m] of packed
// entries (knn_update_kernels.hip).  The class bytes come up; the host makes the ascending lists of the added rows and of the rows to
// search (added and kept-dirty: they lost a neighbour whose replacement is unknown, or never had a list).  Those are answered by the
// build's own step loop (knn_search_steps) and scattered into the working table; the kept-clean rows are joined against the added
// rows, staged in blocks of kKnnUpdBlock, one block after another; the working table goes up as global ids and sims.  A map that is
// not monotone, too many added rows or a shape the join does not cover turn the call into a rebuild: every live row is searched.
// Everything the call allocates it frees.
#include <algorithm>
#include <vector>

#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

namespace {

struct UpdScratch {   // released on every return path
    void* block = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr, j0 = nullptr, j1 = nullptr;
    ~UpdScratch() {
        for (hipEvent_t e : {t0, t1, j0, j1})
            if (e) (void)hipEventDestroy(e);
        if (block) (void)hipFree(block);
    }
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

SearchError VectorIndex::knn_update_check_map(const uint32_t* new_to_old, uint64_t old_len) const {
    if (!new_to_old) {
        if (old_len != nrows_)
            return make_error(FSGPU_ERR_INVALID_CONFIG, "without a map the old table must have record_count rows (old_len " +
                                                            std::to_string(old_len) + ", record_count " + std::to_string(nrows_) + ")");
        return ok();
    }
    std::vector<uint64_t> named((size_t)((old_len + 63) / 64), 0ull);
    for (uint64_t x = 0; x < nrows_; ++x) {
        const uint32_t p = new_to_old[x];
        if (p == kKnnPadRow) continue;
        if (p >= old_len)
            return make_error(FSGPU_ERR_INVALID_CONFIG, "new_to_old[" + std::to_string(x) + "] = " + std::to_string(p) + " is not below old_len");
        uint64_t& w = named[p >> 6];
        if ((w >> (p & 63)) & 1ull)
            return make_error(FSGPU_ERR_INVALID_CONFIG, "two current rows name old row " + std::to_string(p) + " as their predecessor");
        w |= 1ull << (p & 63);
    }
    return ok();
}

SearchError VectorIndex::update_knn_graph(uint32_t m, const uint32_t* old_rows, const float* old_sims, uint64_t old_len, uint32_t old_row_base,
                                          const uint32_t* new_to_old, float max_added_fraction, uint32_t* out_rows, float* out_sims,
                                          KnnUpdateStats* stats) {
    if (stats) *stats = KnnUpdateStats{};
    last_knn_build = KnnBuildStats{};
    if (m < 1 || m > kKnnMaxM) return make_error(FSGPU_ERR_INVALID_CONFIG, "m must be 1 .. 63 (k = m + 1 stays inside the fused tiers)");
    if (!old_rows || !old_sims || !out_rows || !out_sims) return make_error(FSGPU_ERR_INVALID_CONFIG, "the tables and the outputs must not be null");
    if (old_len >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "the old table's ids are 32 bits wide");
    if (tickets_taken() != 0 || lone_.kind != kLoneNone)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun search is outstanding on this index: end it first (the update takes both tickets)");
    FSGPU_TRY(knn_update_check_map(new_to_old, old_len));
    const uint64_t n = nrows_;
    if (n == 0) return ok();
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    FSGPU_TRY(fetch_live_host());
    FSGPU_HIP(hipSetDevice(device_));

    // the predecessors of the rows that have one must increase: ties among kept rows then break as they did
    bool monotone = true;
    if (new_to_old) {
        int64_t prev = -1;
        for (uint64_t x = 0; x < n && monotone; ++x) {
            if (new_to_old[x] == kKnnPadRow) continue;
            if ((int64_t)new_to_old[x] <= prev) monotone = false;
            prev = (int64_t)new_to_old[x];
        }
    }
    const bool join_covers = dim_ <= kKnnUpdMaxDim && dense_rows();

    // one block: old rows | old sims | map | inverse | classes | working table | out rows | out sims | added list | staged block |
    // its global ids | the output kernel's counts
    const size_t old_bytes = (size_t)old_len * m * 4, out_bytes = (size_t)n * m * 4;
    const uint32_t out_blocks = knn_update_output_blocks(n, m);
    const size_t o_osims = align256(old_bytes), o_map = align256(o_osims + old_bytes), o_inv = align256(o_map + (new_to_old ? (size_t)n * 4 : 0)),
                 o_cls = align256(o_inv + (new_to_old ? (size_t)old_len * 4 : 0)), o_work = align256(o_cls + (size_t)n),
                 o_rows = align256(o_work + 2 * out_bytes), o_sims = align256(o_rows + out_bytes), o_added = align256(o_sims + out_bytes),
                 o_stage = align256(o_added + (size_t)n * 4), o_ids = align256(o_stage + (size_t)kKnnUpdBlock * dim_ * 4),
                 o_cnt = align256(o_ids + (size_t)kKnnUpdBlock * 4), bytes = align256(o_cnt + (size_t)out_blocks * 4);
    UpdScratch sc;
    if (hipMalloc(&sc.block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return make_error(FSGPU_ERR_DEVICE, "the k-NN update needs " + std::to_string(bytes) + " bytes of device memory");
    }
    for (hipEvent_t* e : {&sc.t0, &sc.t1, &sc.j0, &sc.j1}) FSGPU_HIP(hipEventCreate(e));
    unsigned char* dev = static_cast<unsigned char*>(sc.block);
    u64* work = reinterpret_cast<u64*>(dev + o_work);
    uint8_t* cls_dev = dev + o_cls;

    FSGPU_HIP(hipEventRecord(sc.t0, stream_));
    if (old_bytes) {
        FSGPU_HIP(hipMemcpyAsync(dev, old_rows, old_bytes, hipMemcpyHostToDevice, stream_));
        FSGPU_HIP(hipMemcpyAsync(dev + o_osims, old_sims, old_bytes, hipMemcpyHostToDevice, stream_));
    }
    KnnUpdClassifyArgs ca{};
    ca.old_rows = reinterpret_cast<const uint32_t*>(dev);
    ca.old_sims = reinterpret_cast<const float*>(dev + o_osims);
    ca.old_len = old_len;
    ca.old_row_base = old_row_base;
    if (new_to_old) {
        FSGPU_HIP(hipMemcpyAsync(dev + o_map, new_to_old, (size_t)n * 4, hipMemcpyHostToDevice, stream_));
        if (old_len) FSGPU_HIP(hipMemsetAsync(dev + o_inv, 0xff, (size_t)old_len * 4, stream_));
        FSGPU_HIP(launch_knn_update_inverse(reinterpret_cast<const uint32_t*>(dev + o_map), n, old_len, reinterpret_cast<uint32_t*>(dev + o_inv),
                                            stream_));
        ca.new_to_old = reinterpret_cast<const uint32_t*>(dev + o_map);
        ca.inv = reinterpret_cast<const uint32_t*>(dev + o_inv);
    }
    ca.live = reinterpret_cast<const u64*>(live_dev_);
    ca.n = n;
    ca.m = m;
    ca.all_dirty = monotone ? 0u : 1u;
    ca.cls = cls_dev;
    ca.work = work;
    FSGPU_HIP(launch_knn_update_classify(ca, stream_));
    std::vector<uint8_t> cls((size_t)n);
    FSGPU_HIP(hipMemcpyAsync(cls.data(), cls_dev, (size_t)n, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));

    // the one N-byte host step: the counts and the ascending lists
    KnnUpdateStats st;
    st.rows = n;
    std::vector<uint32_t> added, searched;
    for (uint64_t x = 0; x < n; ++x) {
        switch (cls[(size_t)x]) {
            case kKnnUpdDead: ++st.dead; break;
            case kKnnUpdAdded: ++st.added; added.push_back((uint32_t)x); break;
            case kKnnUpdClean: ++st.kept_clean; break;
            default: ++st.kept_dirty; break;
        }
    }
    if (!monotone) st.rebuilt = 1;
    else if (!join_covers) st.rebuilt = 3;
    else if ((double)st.added > (double)max_added_fraction * (double)n) st.rebuilt = 2;
    const bool rebuild = st.rebuilt != 0;
    searched.reserve((size_t)(rebuild ? n - st.dead : st.added + st.kept_dirty));
    for (uint64_t x = 0; x < n; ++x) {
        const uint8_t c = cls[(size_t)x];
        if (rebuild ? c != kKnnUpdDead : (c == kKnnUpdAdded || c == kKnnUpdDirty)) searched.push_back((uint32_t)x);
    }
    st.searched_sources = searched.size();

    // ---- the full searches: the build's step loop over the list, its lists scattered into the working table ----
    if (!searched.empty()) {
        size_t next = 0;
        auto next_chunk = [&](std::vector<uint32_t>& src, uint32_t cap) {
            const size_t take = std::min<size_t>(cap, searched.size() - next);
            src.insert(src.end(), searched.begin() + (ptrdiff_t)next, searched.begin() + (ptrdiff_t)(next + take));
            next += take;
            return next < searched.size();
        };
        auto sink = [&](const KnnStepLists& l) -> SearchError {
            KnnUpdScatterArgs s{};
            s.src = l.src_dev;
            s.rows = l.rows_dev;
            s.sims = l.sims_dev;
            s.n = l.n;
            s.m = m;
            s.row_base = (uint32_t)row_base_;
            s.nrows = n;
            s.work = work;
            FSGPU_HIP(launch_knn_update_scatter(s, l.stream));
            return ok();
        };
        FSGPU_TRY(knn_search_steps((uint32_t)std::min<size_t>(kKnnChunk, searched.size()), m, true, false, next_chunk, sink));
    }

    // ---- the join: kept-clean rows x added rows, one staged block after another ----
    if (!rebuild && !added.empty() && st.kept_clean) {
        st.join_pairs = st.kept_clean * st.added;
        FSGPU_HIP(hipMemcpyAsync(dev + o_added, added.data(), added.size() * 4, hipMemcpyHostToDevice, stream_));
        FSGPU_HIP(hipEventRecord(sc.j0, stream_));
        for (size_t b0 = 0; b0 < added.size(); b0 += kKnnUpdBlock) {
            const uint32_t nb = (uint32_t)std::min<size_t>(kKnnUpdBlock, added.size() - b0);
            KnnStageArgs sa{};
            sa.slab = slab_dev_;
            sa.row_stride = row_stride_ ? row_stride_ : dim_ * (f32_ ? 4u : 2u);
            sa.dim = dim_;
            sa.slab_f32 = f32_ ? 1u : 0u;
            sa.row_base = (uint32_t)row_base_;
            sa.src_local = reinterpret_cast<const uint32_t*>(dev + o_added) + b0;
            sa.n = nb;
            sa.queries = reinterpret_cast<float*>(dev + o_stage);
            sa.src_out = reinterpret_cast<uint32_t*>(dev + o_ids);
            FSGPU_HIP(launch_knn_stage_rows(sa, stream_));
            KnnUpdJoinArgs ja{};
            ja.slab = slab_dev_;
            ja.row_stride = sa.row_stride;
            ja.dim = dim_;
            ja.slab_f32 = sa.slab_f32;
            ja.hreduce = hreduce;
            ja.m = m;
            ja.cls = cls_dev;
            ja.work = work;
            ja.added = sa.queries;
            ja.added_rows = sa.src_local;
            ja.n_added = nb;
            for (uint64_t r0 = 0; r0 < n; r0 += kKnnUpdLaunchRows) {
                ja.row0 = (uint32_t)r0;
                ja.nrows = (uint32_t)std::min<uint64_t>(kKnnUpdLaunchRows, n - r0);
                FSGPU_HIP(launch_knn_update_join(ja, stream_));
            }
        }
        FSGPU_HIP(hipEventRecord(sc.j1, stream_));
    }

    // ---- the working table -> global ids and sims ----
    KnnUpdOutputArgs oa{};
    oa.work = work;
    oa.cls = cls_dev;
    oa.n = n;
    oa.m = m;
    oa.row_base = (uint32_t)row_base_;
    oa.out_rows = reinterpret_cast<uint32_t*>(dev + o_rows);
    oa.out_sims = reinterpret_cast<float*>(dev + o_sims);
    oa.join_entries = reinterpret_cast<uint32_t*>(dev + o_cnt);
    FSGPU_HIP(launch_knn_update_output(oa, stream_));
    std::vector<uint32_t> counts(out_blocks);
    FSGPU_HIP(hipMemcpyAsync(out_rows, oa.out_rows, out_bytes, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipMemcpyAsync(out_sims, oa.out_sims, out_bytes, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipMemcpyAsync(counts.data(), oa.join_entries, (size_t)out_blocks * 4, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipEventRecord(sc.t1, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    for (uint32_t c : counts) st.join_entries += c;
    float ms = 0.0f;
    FSGPU_HIP(hipEventElapsedTime(&ms, sc.t0, sc.t1));
    st.device_ms = ms;
    if (st.join_pairs) {
        FSGPU_HIP(hipEventElapsedTime(&ms, sc.j0, sc.j1));
        st.join_ms = ms;
    }
    if (stats) *stats = st;
    return ok();
}

}  // namespace fsgpu

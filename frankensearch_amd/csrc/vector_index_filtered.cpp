// vector_index_filtered.cpp — a batched, row-level search in which every query names its own resident filter, or none.
// The reference takes `Option<&dyn SearchFilter>` per search (crates/frankensearch-core/src/filter.rs:19-56) and scores only the
// allowed rows when a filter lets through fewer than 1/GATHER_SELECTIVITY_DIVISOR of the corpus (search.rs:1114-1255, 1667).  Here:
//   plan (host) -> queries gathered into group order -> selective groups: ONE segmented gather scan + ONE merge;
//   unfiltered / dense groups: search_top_k_batched_device each -> hits scattered back into batch order.
// Kernels: filter_gather_kernels.hip; the merge, the query gather and the hit scatter are scan_kernels.hip's.
#include "vector_index.hpp"

#include <algorithm>
#include <cstring>
#include <vector>

#include "../../include/fsgpu.h"
#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

SearchError multi_filter_plan(uint64_t nrows, const uint64_t* allowed_per_filter, uint32_t nfilters, const int32_t* filter_of_query,
                              uint32_t nq, int32_t* out_group_of_query, int32_t* out_path_of_group, int32_t* out_filter_of_group,
                              uint32_t* out_ngroups) {
    for (uint32_t q = 0; q < nq; ++q)
        if (filter_of_query[q] < -1 || (filter_of_query[q] >= 0 && (uint32_t)filter_of_query[q] >= nfilters))
            return make_error(FSGPU_ERR_INVALID_CONFIG, "filter_of_query[" + std::to_string(q) + "] = " + std::to_string(filter_of_query[q]) +
                                                            " names none of the " + std::to_string(nfilters) + " filters");
    std::vector<int32_t> group_of_filter((size_t)nfilters + 1, -1);   // slot 0: no filter
    uint32_t ngroups = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        const int32_t f = filter_of_query[q];
        int32_t& g = group_of_filter[(size_t)(f + 1)];
        if (g < 0) {
            g = (int32_t)ngroups++;
            int32_t path = kMultiUnfiltered;
            if (f >= 0 && allowed_per_filter) {   // (without the counts the call only checks the indices)
                const uint64_t allowed = allowed_per_filter[f];
                // GATHER_SELECTIVITY_DIVISOR = 50 (search.rs:1667, 1136-1139): allowed * 50 < nrows, in 128 bits (no overflow at any count)
                const bool selective = (unsigned __int128)allowed * 50u < (unsigned __int128)nrows;
                path = allowed == 0 ? kMultiEmpty : selective ? kMultiGather : kMultiDense;
            }
            if (out_path_of_group) out_path_of_group[g] = path;
            if (out_filter_of_group) out_filter_of_group[g] = f;
        }
        if (out_group_of_query) out_group_of_query[q] = g;
    }
    if (out_ngroups) *out_ngroups = ngroups;
    return ok();
}

SearchError build_filter_row_list(int device, const uint64_t* words_dev, uint64_t nrows, uint64_t allowed, DeviceBuffer* rows) {
    if (nrows > 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row lists serve indexes of fewer than 2^32 rows");
    FSGPU_HIP(hipSetDevice(device));
    FSGPU_TRY(rows->reserve((size_t)std::max<uint64_t>(allowed, 1) * 4));
    if (allowed == 0 || nrows == 0) return ok();
    DeviceBuffer scratch;
    SearchError e = scratch.reserve(filter_row_list_scratch_bytes((uint32_t)nrows));
    if (!e.ok()) return e;
    const size_t nwords = (size_t)((nrows + 63) / 64), nblocks = (nwords + kRowListWordsPerBlock - 1) / kRowListWordsPerBlock;
    uint32_t* s = static_cast<uint32_t*>(scratch.ptr);
    hipError_t h = launch_filter_row_list(reinterpret_cast<const u64*>(words_dev), (uint32_t)nrows, (uint32_t)allowed, s,
                                          static_cast<uint32_t*>(rows->ptr), s + nwords + nblocks, nullptr);
    uint32_t total = 0;
    if (h == hipSuccess) h = hipMemcpy(&total, s + nwords + nblocks, 4, hipMemcpyDeviceToHost);   // (blocks behind the kernels)
    scratch.release();
    if (h != hipSuccess) return hip_fail(h, "build_filter_row_list");
    if (total != allowed) return make_error(FSGPU_ERR_DEVICE, "the device-built row list does not match the bitmap's popcount");
    return ok();
}

SearchError VectorIndex::search_top_k_multi_filtered(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                                     const ResidentFilterView* filters, uint32_t nfilters, const int32_t* filter_of_query,
                                                     uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                                     hipStream_t stream, uint32_t* fallbacks) {
    if (fallbacks) *fallbacks = 0;
    // ---- validation: nothing is launched before all of it has passed ----
    FSGPU_TRY(ensure_query_dimension(query_len));
    if (nq == 0) return ok();
    std::vector<uint64_t> allowed(nfilters);
    for (uint32_t f = 0; f < nfilters; ++f) allowed[f] = filters[f].allowed;
    std::vector<int32_t> group_of_query(nq), path_of_group((size_t)nfilters + 1), filter_of_group((size_t)nfilters + 1);
    uint32_t ngroups = 0;
    FSGPU_TRY(multi_filter_plan(nrows_, allowed.data(), nfilters, filter_of_query, nq, group_of_query.data(), path_of_group.data(),
                                filter_of_group.data(), &ngroups));
    FSGPU_HIP(hipSetDevice(device_));
    if (k == 0 || nrows_ == 0) {   // search.rs:437-439
        FSGPU_HIP(hipMemsetAsync(out_counts_dev, 0, (size_t)nq * 4, stream));
        FSGPU_HIP(hipStreamSynchronize(stream));
        return ok();
    }
    // ---- group order: the gather groups first (their slots are one block for the scan and the merge), then the others ----
    const bool gather_ok = !f32_ && dense_rows() && nrows_ <= 0xffffffffull && filter_gather_supported(dim_, k);
    std::vector<uint32_t> group_size(ngroups, 0), group_first(ngroups, 0), order;   // order: groups as their slots follow each other
    for (uint32_t q = 0; q < nq; ++q) ++group_size[group_of_query[q]];
    for (int pass = 0; pass < 2; ++pass)
        for (uint32_t g = 0; g < ngroups; ++g)
            if ((path_of_group[g] == kMultiGather && gather_ok) == (pass == 0)) order.push_back(g);
    uint32_t slots = 0, gather_slots = 0, gather_groups = 0;
    for (uint32_t g : order) {
        group_first[g] = slots;
        slots += group_size[g];
        if (path_of_group[g] == kMultiGather && gather_ok) {
            gather_slots = slots;
            ++gather_groups;
        }
    }
    // ---- one device block: query index per slot | group descriptors | grouped queries | grouped rows | scores | counts ----
    auto align_up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
    const size_t o_idx = 0, o_desc = align_up((size_t)nq * 4, 256), o_q = align_up(o_desc + (size_t)gather_groups * sizeof(FilterGatherGroup), 256),
                 o_rows = align_up(o_q + (size_t)nq * dim_ * 4, 256), o_scores = align_up(o_rows + (size_t)nq * k * 4, 256),
                 o_counts = align_up(o_scores + (size_t)nq * k * 4, 256), total = align_up(o_counts + (size_t)nq * 4, 256);
    FSGPU_TRY(ws_multi_.reserve(total));
    unsigned char* base = static_cast<unsigned char*>(ws_multi_.ptr);
    uint32_t* idx_dev = reinterpret_cast<uint32_t*>(base + o_idx);
    FilterGatherGroup* desc_dev = reinterpret_cast<FilterGatherGroup*>(base + o_desc);
    float* gq = reinterpret_cast<float*>(base + o_q);
    uint32_t* g_rows = reinterpret_cast<uint32_t*>(base + o_rows);
    float* g_scores = reinterpret_cast<float*>(base + o_scores);
    uint32_t* g_counts = reinterpret_cast<uint32_t*>(base + o_counts);
    multi_host_.assign(o_q, 0);
    uint32_t* idx_host = reinterpret_cast<uint32_t*>(multi_host_.data() + o_idx);
    FilterGatherGroup* desc_host = reinterpret_cast<FilterGatherGroup*>(multi_host_.data() + o_desc);
    {
        std::vector<uint32_t> fill(group_first);
        for (uint32_t q = 0; q < nq; ++q) idx_host[fill[group_of_query[q]]++] = q;   // ascending query order inside a group
    }
    // blocks per gather group: over all groups about four per CU (two are resident) — a block that walks many tiles sorts a query's
    // list once, behind its last tile, and after the first tiles few rows beat what it holds —, few enough that a query's lists fit the
    // merge's one-pass form (16,384 entries), never more than the group has tiles
    uint32_t grid_x = 0;
    const uint32_t list_stride = k <= 64 ? 64 : k;
    if (gather_groups) {
        const uint32_t by_device = std::min<uint32_t>(1024, std::max<uint32_t>(8, (uint32_t)(4 * num_cus_) / gather_groups));
        const uint32_t cap = std::max<uint32_t>(1, std::min<uint32_t>(by_device, 16384 / k));
        uint32_t d = 0;
        for (uint32_t g : order) {
            if (!(path_of_group[g] == kMultiGather && gather_ok)) continue;
            const ResidentFilterView& f = filters[filter_of_group[g]];
            if (!f.rows_dev) return make_error(FSGPU_ERR_INVALID_CONFIG, "a selective filter came without its row list");
            FilterGatherGroup& gd = desc_host[d++];
            gd.rows = f.rows_dev;
            gd.n = (uint32_t)f.allowed;
            gd.q0 = group_first[g];
            gd.nq = group_size[g];
            gd.nblocks = std::min<uint32_t>((gd.n + kGatherTileRows - 1) / kGatherTileRows, cap);
            grid_x = std::max(grid_x, gd.nblocks);
        }
        FSGPU_TRY(ws_multi_lists_.reserve((size_t)gather_slots * grid_x * list_stride * 8));
    }
    FSGPU_HIP(hipMemcpyAsync(base, multi_host_.data(), o_q, hipMemcpyHostToDevice, stream));
    FSGPU_HIP(hipMemsetAsync(g_rows, 0xff, (size_t)nq * k * 4, stream));
    FSGPU_HIP(hipMemsetAsync(g_scores, 0xff, (size_t)nq * k * 4, stream));
    FSGPU_HIP(hipMemsetAsync(g_counts, 0, (size_t)nq * 4, stream));   // (an empty filter's queries: nothing else writes their slots)
    FSGPU_HIP(launch_gather_queries(queries_dev, idx_dev, nq, dim_, dim_, gq, stream));
    if (gather_groups) {
        FilterGatherArgs a;
        a.slab = slab_dev_;
        a.live = reinterpret_cast<const u64*>(live_dev_);
        a.queries = gq;
        a.groups = desc_dev;
        a.partial = static_cast<u64*>(ws_multi_lists_.ptr);
        a.list_stride = list_stride;
        a.nrows = (uint32_t)nrows_;
        a.dim = dim_;
        a.k = k;
        a.row_base = (uint32_t)row_base_;
        a.row_stride = row_stride_ ? row_stride_ : dim_ * 2;
        a.hreduce = hreduce;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        if (profiling) {   // fsgpu_index_set_profiling: the gather launch alone between two events (fsgpu_index_scan_stats)
            FSGPU_HIP(hipEventCreate(&e0));
            FSGPU_HIP(hipEventCreate(&e1));
            FSGPU_HIP(hipEventRecord(e0, stream));
        }
        constexpr uint32_t kMaxGridY = 65535;   // (one launch unless a call names more selective filters than a grid has rows)
        for (uint32_t g0 = 0; g0 < gather_groups; g0 += kMaxGridY) {
            a.groups = desc_dev + g0;
            FSGPU_HIP(launch_filter_gather_scan(a, std::min(gather_groups - g0, kMaxGridY), grid_x, stream));
        }
        if (profiling) {
            FSGPU_HIP(hipEventRecord(e1, stream));
            events_.emplace_back(e0, e1);
            for (uint32_t d = 0; d < gather_groups; ++d) profiled_rows_ += desc_host[d].n;   // rows staged: the sum of the lists
        }
        MergeArgs m;
        m.lists = a.partial;
        m.q_stride = (uint64_t)grid_x * list_stride;
        m.l_stride = list_stride;
        m.nlists = grid_x;
        m.list_len = k;
        m.k = k;
        m.out_stride = k;
        m.out_rows = g_rows;
        m.out_scores = g_scores;
        m.out_counts = g_counts;
        m.out_packed = nullptr;
        FSGPU_HIP(launch_merge_topk(m, (int)gather_slots, stream));
        multi_gathered += gather_slots;
    }
    uint32_t fb_total = 0;
    std::vector<uint32_t> per_query;   // groups left to the per-query filtered search
    for (uint32_t g : order) {
        const int32_t path = path_of_group[g];
        if (path == kMultiEmpty || (path == kMultiGather && gather_ok)) continue;
        if (path == kMultiGather) {
            per_query.push_back(g);
            continue;
        }
        const uint32_t s0 = group_first[g], n = group_size[g];
        const uint64_t* allow_dev = path == kMultiDense ? filters[filter_of_group[g]].words_dev : nullptr;
        uint32_t fb = 0;
        FSGPU_TRY(search_top_k_batched_device(gq + (size_t)s0 * dim_, n, query_len, k, allow_dev, g_rows + (size_t)s0 * k,
                                              g_scores + (size_t)s0 * k, g_counts + s0, stream, &fb));
        fb_total += fb;
        (path == kMultiDense ? multi_scanned : multi_unfiltered) += n;
    }
    FSGPU_HIP(launch_scatter_hits(idx_dev, nq, k, g_rows, g_scores, g_counts, out_rows_dev, out_scores_dev, out_counts_dev, nullptr, stream));
    FSGPU_HIP(hipStreamSynchronize(stream));
    // ---- selective groups of a shape the gather scan does not cover: the per-query filtered search, one query at a time ----
    if (!per_query.empty()) {
        std::vector<float> q1(dim_), s1(k);
        std::vector<uint32_t> r1(k);
        for (uint32_t g : per_query) {
            const ResidentFilterView& f = filters[filter_of_group[g]];
            for (uint32_t s = group_first[g]; s < group_first[g] + group_size[g]; ++s) {
                const uint32_t q = idx_host[s];
                uint32_t c1 = 0;
                FSGPU_HIP(hipMemcpy(q1.data(), queries_dev + (size_t)q * dim_, (size_t)dim_ * 4, hipMemcpyDeviceToHost));
                std::fill(r1.begin(), r1.end(), 0xffffffffu);
                std::memset(s1.data(), 0xff, (size_t)k * 4);
                FSGPU_TRY(search_top_k(q1.data(), 1, query_len, k, f.words_host, r1.data(), s1.data(), &c1, f.words_dev));
                FSGPU_HIP(hipMemcpy(out_rows_dev + (size_t)q * k, r1.data(), (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_scores_dev + (size_t)q * k, s1.data(), (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_counts_dev + q, &c1, 4, hipMemcpyHostToDevice));
                ++fb_total;
                ++multi_fallbacks;
            }
        }
    }
    if (fallbacks) *fallbacks = fb_total;
    return ok();
}

SearchError VectorIndex::search_top_k_multi_filtered_host(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                          const ResidentFilterView* filters, uint32_t nfilters,
                                                          const int32_t* filter_of_query, uint32_t* out_rows, float* out_scores,
                                                          uint32_t* out_counts, uint32_t* fallbacks) {
    if (fallbacks) *fallbacks = 0;
    FSGPU_TRY(ensure_query_dimension(query_len));
    if (nq == 0) return ok();
    FSGPU_TRY(multi_filter_plan(nrows_, nullptr, nfilters, filter_of_query, nq, nullptr, nullptr, nullptr, nullptr));   // indices only
    FSGPU_HIP(hipSetDevice(device_));
    auto align_up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
    const size_t kk = std::max<uint32_t>(k, 1);
    const size_t o_rows = align_up((size_t)nq * dim_ * 4, 256), o_scores = align_up(o_rows + (size_t)nq * kk * 4, 256),
                 o_counts = align_up(o_scores + (size_t)nq * kk * 4, 256), total = align_up(o_counts + (size_t)nq * 4, 256);
    FSGPU_TRY(ws_multi_io_.reserve(total));
    unsigned char* base = static_cast<unsigned char*>(ws_multi_io_.ptr);
    FSGPU_HIP(hipMemcpyAsync(base, queries, (size_t)nq * dim_ * 4, hipMemcpyHostToDevice, stream_));
    FSGPU_TRY(search_top_k_multi_filtered(reinterpret_cast<const float*>(base), nq, query_len, k, filters, nfilters, filter_of_query,
                                          reinterpret_cast<uint32_t*>(base + o_rows), reinterpret_cast<float*>(base + o_scores),
                                          reinterpret_cast<uint32_t*>(base + o_counts), stream_, fallbacks));
    if (k == 0 || nrows_ == 0) {
        for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
        return ok();
    }
    return fetch_batched_results(base, o_rows, o_scores, o_counts, total, nq, k, out_rows, out_scores, out_counts);
}

}  // namespace fsgpu

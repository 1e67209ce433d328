// vector_index_knn_optimize.cpp — the graph optimisation over a neighbour table of a VectorIndex (include/fsgpu.h,
// fsgpu_knn_graph_optimize).  The index supplies the device, the stream and row_base and nothing else: the table goes
// down in one copy, the detour kernel writes F, `degree` rounds (keys, sort, place, advance) collect the reverse candidates in
// (rank, source) order, the merge kernel writes the lists, which come up in one copy.  Everything the call allocates it frees.
#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

namespace {

struct OptScratch {   // released on every return path
    void* block = nullptr;
    hipEvent_t t0 = nullptr, t1 = nullptr;
    ~OptScratch() {
        if (t0) (void)hipEventDestroy(t0);
        if (t1) (void)hipEventDestroy(t1);
        if (block) (void)hipFree(block);
    }
};

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

}  // namespace

SearchError VectorIndex::optimize_knn_graph(const uint32_t* graph_rows, uint32_t width, uint32_t degree, uint32_t* out_rows,
                                            KnnOptimizeStats* stats) {
    if (stats) *stats = KnnOptimizeStats{};
    if (degree < 1 || degree > width || width > kKnnOptMaxWidth)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the degree must be 1 .. width and the width at most 64");
    if (tickets_taken() != 0 || lone_.kind != kLoneNone)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "a begun search is outstanding on this index: end it first");
    const uint64_t n = nrows_;
    if (n == 0) return ok();
    if (!graph_rows || !out_rows) return make_error(FSGPU_ERR_INVALID_CONFIG, "the table and the output must not be null");
    if (n > 0xfffffffeull) return make_error(FSGPU_ERR_INVALID_CONFIG, "the table's ids are 32 bits wide");
    FSGPU_HIP(hipSetDevice(device_));

    size_t sort_bytes = 0;
    FSGPU_HIP(sort_keys_desc_temp_bytes((size_t)n, &sort_bytes));
    // one block: table | F | reverse candidates | out | keys | sorted | sort scratch | advance | fill | seen before, after | counters
    const size_t list_bytes = (size_t)n * degree * 4;
    const size_t o_fwd = align256((size_t)n * width * 4), o_rev = align256(o_fwd + list_bytes), o_out = align256(o_rev + list_bytes),
                 o_keys = align256(o_out + list_bytes), o_sorted = align256(o_keys + (size_t)n * 8), o_sort = align256(o_sorted + (size_t)n * 8),
                 o_adv = align256(o_sort + sort_bytes), o_fill = align256(o_adv + (size_t)n * 4), o_seen = align256(o_fill + (size_t)n * 4),
                 o_cnt = align256(o_seen + (stats ? 2 * (size_t)n : 0)), bytes = o_cnt + 256;
    OptScratch sc;
    if (hipMalloc(&sc.block, bytes) != hipSuccess) {
        (void)hipGetLastError();
        return make_error(FSGPU_ERR_DEVICE, "the graph optimisation needs " + std::to_string(bytes) + " bytes of device memory");
    }
    FSGPU_HIP(hipEventCreate(&sc.t0));
    FSGPU_HIP(hipEventCreate(&sc.t1));
    unsigned char* dev = static_cast<unsigned char*>(sc.block);
    uint32_t* fill = reinterpret_cast<uint32_t*>(dev + o_fill);
    u64* counters = reinterpret_cast<u64*>(dev + o_cnt);   // F entries, reverse entries, zero before, zero after, max detour count

    FSGPU_HIP(hipMemcpyAsync(dev, graph_rows, (size_t)n * width * 4, hipMemcpyHostToDevice, stream_));
    FSGPU_HIP(hipEventRecord(sc.t0, stream_));
    // fill .. counters: the placed counts start at 0, as do the seen flags and the counters
    FSGPU_HIP(hipMemsetAsync(fill, 0, bytes - o_fill, stream_));

    KnnOptDetourArgs da{};
    da.table = reinterpret_cast<const uint32_t*>(dev);
    da.n = n;
    da.width = width;
    da.degree = degree;
    da.row_base = (uint32_t)row_base_;
    da.fwd = reinterpret_cast<uint32_t*>(dev + o_fwd);
    da.max_detour = stats ? reinterpret_cast<uint32_t*>(counters + 4) : nullptr;
    da.seen_before = stats ? dev + o_seen : nullptr;
    FSGPU_HIP(launch_knn_opt_detour(da, stream_));

    KnnOptRoundArgs ra{};
    ra.fwd = da.fwd;
    ra.n = n;
    ra.degree = degree;
    ra.row_base = da.row_base;
    ra.keys = reinterpret_cast<u64*>(dev + o_keys);
    ra.sorted = reinterpret_cast<u64*>(dev + o_sorted);
    ra.advance = reinterpret_cast<uint32_t*>(dev + o_adv);
    ra.fill = fill;
    ra.rev = reinterpret_cast<uint32_t*>(dev + o_rev);
    for (uint32_t r = 0; r < degree; ++r) {
        ra.rank = r;
        FSGPU_HIP(launch_knn_opt_round(ra, dev + o_sort, sort_bytes, stream_));
    }

    KnnOptMergeArgs ma{};
    ma.fwd = da.fwd;
    ma.rev = ra.rev;
    ma.fill = fill;
    ma.n = n;
    ma.degree = degree;
    ma.row_base = da.row_base;
    ma.out = reinterpret_cast<uint32_t*>(dev + o_out);
    ma.edge_counts = stats ? counters : nullptr;
    ma.seen_after = stats ? dev + o_seen + n : nullptr;
    FSGPU_HIP(launch_knn_opt_merge(ma, stream_));
    if (stats) FSGPU_HIP(launch_knn_opt_count_zero(dev + o_seen, dev + o_seen + n, n, counters + 2, stream_));
    FSGPU_HIP(hipEventRecord(sc.t1, stream_));

    u64 host_counters[5] = {0, 0, 0, 0, 0};
    if (stats) FSGPU_HIP(hipMemcpyAsync(host_counters, counters, sizeof(host_counters), hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipMemcpyAsync(out_rows, dev + o_out, list_bytes, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    if (stats) {
        float ms = 0.0f;
        FSGPU_HIP(hipEventElapsedTime(&ms, sc.t0, sc.t1));
        stats->rows = n;
        stats->forward_edges = host_counters[0];
        stats->reverse_edges = host_counters[1];
        stats->zero_in_degree_before = host_counters[2];
        stats->zero_in_degree_after = host_counters[3];
        stats->max_detour_count = (uint32_t)host_counters[4];
        stats->device_ms = ms;
    }
    return ok();
}

}  // namespace fsgpu

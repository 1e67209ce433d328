// ivf_index.cpp — the host side of the inverted-file index (ivf_index.hpp; include/fsgpu.h, "IVF index").
//
// BUILD.  The training rows' gate and the strided initial rows are worked out on the host from the live bitmap; everything else
// runs on the index's stream: per Lloyd iteration an assignment (ivf_assign_kernel over ranges of kIvfLaunchRows rows), the lists
// (keys, the library's radix sort, boundaries) and the centroid update; then the assignment of ALL live rows and their lists.
// SEARCH.  (1) the coarse step, k = nprobe over the centroid matrix: an internal F32 index in the parent's hreduce order answers it
// (its batched search; below 32,768 rows that is the exact F32 kernels, a few queries per pass) — or, for 16 queries and more and
// nprobe <= 63, ONE launch of the exact transposed join (knn_update_kernels.hip: the queries are its f32 "slab" rows in LDS, the
// centroids stream past them, a query's running list is its nprobe best); dot_product_f32_bytes_f32 is symmetric in its operands
// bit for bit — every product commutes and the order of the additions depends on the element index alone — and both keep the
// total order, so the two ways agree to the bit; (2) one small copy of the coarse rows to the host, where the plan is made: the
// (list, query) pairs by list, then by query, one FilterGatherGroup per probed list with members, the slot -> query map, per query
// the slots of its pairs; (3) ONE launch of the segmented gather scan and merge_topk over its blocks' lists; (4) the per-query
// merge; (5) one copy of counts and hits into a pinned block.  Only when some count is below k is the live count taken and the
// fallback considered.
// THE LIST FILTER (opt-in) sits between (2) and (3): the probed lists are scored on the int8 matrix cores from the
// handle's cluster-ordered copy, a selection keeps per slot the rows that can still reach its exact top k, and a second plan
// (ivf_filter_plan.hpp) hands (3) the candidates in the place of the lists.  (3), (4) and (5) run as they are.
#include "ivf_index.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

#include "../../include/fsgpu.h"
#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

namespace {

size_t align256(size_t v) { return (v + 255) / 256 * 256; }

struct StageTimer {   // one stage between two events on the stream; the stop waits (a build is not a latency path)
    hipEvent_t a, b;
    hipStream_t stream;
    hipError_t start() { return hipEventRecord(a, stream); }
    hipError_t stop(double* sum) {
        hipError_t e = hipEventRecord(b, stream);
        if (e != hipSuccess) return e;
        e = hipEventSynchronize(b);
        if (e != hipSuccess) return e;
        float ms = 0.0f;
        e = hipEventElapsedTime(&ms, a, b);
        *sum += ms;
        return e;
    }
};

}  // namespace

// ---- what the handle needs of the index ------------------------------------------------------------------------------------------------

SearchError VectorIndex::ivf_view(IvfSlabView* out) const {
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (f32_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the IVF index serves F16 slabs");
    if (!dense_rows()) return make_error(FSGPU_ERR_INVALID_CONFIG, "the IVF index does not serve a truncated view");
    if (nrows_ + row_base_ >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row ids must fit 32 bits");
    out->slab = slab_dev_;
    out->live = reinterpret_cast<const u64*>(live_dev_);
    out->nrows = (uint32_t)nrows_;
    out->dim = dim_;
    out->row_base = (uint32_t)row_base_;
    out->row_stride = row_stride_ ? row_stride_ : dim_ * 2u;
    out->num_cus = num_cus_;
    return ok();
}

SearchError VectorIndex::ivf_filter_copy(FilterCopyView* out) {
    if (!dense_rows() || nrows_ == 0 || nrows_ > 0xffffffffull)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the int8 filter serves dense, non-empty slabs only");
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(ensure_filter_copy(stream_, true));
    if (!filter_ready()) return make_error(FSGPU_ERR_DEVICE, "no room for the int8 copy of the slab");
    out->slab_i8 = static_cast<const signed char*>(filter_slab());
    out->max_bits = filter_max();
    out->stats = filter_stats();
    out->rotated = i8f_rot_;
    out->rot_mat = i8f_rot_ ? static_cast<const double*>(rot_mat_.ptr) : nullptr;
    out->extra_coeff = i8f_rot_ ? rot_extra_coeff_ : 0.0;
    return ok();
}

// ---- the handle ------------------------------------------------------------------------------------------------------------------------

IvfIndex::~IvfIndex() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    if (ev_begin_) (void)hipEventDestroy(ev_begin_);
    if (ev_end_) (void)hipEventDestroy(ev_end_);
    for (hipEvent_t e : fev_)
        if (e) (void)hipEventDestroy(e);
    for (DeviceBuffer* b : {&ordered_, &filter_words_, &filter_rot_mat_, &fq_, &fscratch_, &fslot_, &fplan_}) b->release();
    if (pin_) (void)hipHostFree(pin_);
    centroids_.release();
    offsets_.release();
    list_rows_.release();
    ws_.release();
    ws_lists_.release();
    coarse_ids_.release();
}

SearchError IvfIndex::init(VectorIndex* index, uint32_t nlist, const float* init_centroids, const IvfConfig& config) {
    VectorIndex::IvfSlabView v;
    FSGPU_TRY(index->ivf_view(&v));
    const uint32_t dim = v.dim;
    if (dim % 8 != 0 || !filter_gather_supported(dim, 1) || !ivf_assign_supported(dim))
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the IVF index serves dimensions that are a multiple of 8 and that the gather scan covers");
    if (nlist < 1 || nlist > kIvfMaxLists) return make_error(FSGPU_ERR_INVALID_CONFIG, "1 <= nlist <= 65,536 does not hold");
    if (config.iters > kIvfMaxIters) return make_error(FSGPU_ERR_INVALID_CONFIG, "iters exceeds 64");
    if (init_centroids)
        for (size_t i = 0; i < (size_t)nlist * dim; ++i)
            if (!std::isfinite(init_centroids[i])) return make_error(FSGPU_ERR_INVALID_CONFIG, "init_centroids holds a non-finite value");
    if (index->device() < 0) return make_error(FSGPU_ERR_NO_DEVICE, "index has no device");
    FSGPU_TRY(index->fetch_live_host());
    const std::vector<uint64_t>& live = index->live_host();
    auto is_live = [&](uint64_t r) { return live.empty() || ((live[r >> 6] >> (r & 63)) & 1ull); };
    // the training rows: the live rows among floor(i * N / n_train), ascending; n_train 0 or >= N: every live row
    const uint64_t n = v.nrows;
    const bool strided = config.n_train != 0 && config.n_train < n;
    std::vector<uint32_t> train_rows;
    train_rows.reserve((size_t)(strided ? config.n_train : n));
    if (strided) {
        for (uint64_t i = 0; i < config.n_train; ++i) {
            const uint64_t r = (uint64_t)(((unsigned __int128)i * n) / config.n_train);
            if (is_live(r)) train_rows.push_back((uint32_t)r);
        }
    } else {
        for (uint64_t r = 0; r < n; ++r)
            if (is_live(r)) train_rows.push_back((uint32_t)r);
    }
    if (nlist > train_rows.size())
        return make_error(FSGPU_ERR_INVALID_CONFIG, "nlist " + std::to_string(nlist) + " exceeds the " + std::to_string(train_rows.size()) + " training rows");

    device_ = index->device();
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_HIP(hipEventCreate(&ev_begin_));
    FSGPU_HIP(hipEventCreate(&ev_end_));
    index_ = index;
    nrows_ = n;
    nlist_ = nlist;
    dim_ = dim;
    cfg_ = config;
    generation_ = index->generation();
    hreduce_ = index->hreduce;
    FSGPU_TRY(train(v, init_centroids, train_rows, !strided));
    // the coarse quantiser: an F32 index over the centroid matrix (not its owner), in the parent's hreduce order
    FSGPU_TRY(coarse_.init_device(device_, dim, nlist, centroids_.ptr, nullptr, 0, true));
    coarse_.hreduce = hreduce_;
    std::vector<uint32_t> ids(nlist);
    for (uint32_t c = 0; c < nlist; ++c) ids[c] = c;
    FSGPU_TRY(coarse_ids_.reserve((size_t)nlist * 4));
    FSGPU_HIP(hipMemcpy(coarse_ids_.ptr, ids.data(), (size_t)nlist * 4, hipMemcpyHostToDevice));
    return ok();
}

SearchError IvfIndex::train(const VectorIndex::IvfSlabView& v, const float* init_centroids, const std::vector<uint32_t>& train_rows,
                            bool train_is_live) {
    hipStream_t stream = index_->stream();
    const uint32_t n = v.nrows, dim = v.dim, nlist = nlist_;
    const size_t words = ((size_t)n + 63) / 64;
    size_t sort_bytes = 0;
    FSGPU_HIP(sort_keys_desc_temp_bytes((size_t)n, &sort_bytes));
    FSGPU_TRY(centroids_.reserve((size_t)nlist * dim * 4));
    FSGPU_TRY(offsets_.reserve(((size_t)nlist + 1) * 8));
    FSGPU_TRY(list_rows_.reserve((size_t)n * 4));
    // the build's block: assign | previous assign | training gate | keys | sorted | sort scratch | initial rows | their ids | counter
    const size_t o_prev = align256((size_t)n * 4), o_gate = align256(o_prev + (size_t)n * 4), o_keys = align256(o_gate + words * 8),
                 o_sorted = align256(o_keys + (size_t)n * 8), o_sort = align256(o_sorted + (size_t)n * 8),
                 o_init = align256(o_sort + sort_bytes), o_init_out = align256(o_init + (size_t)nlist * 4),
                 o_cnt = align256(o_init_out + (size_t)nlist * 4), bytes = o_cnt + 256;
    DeviceBuffer block;
    FSGPU_TRY(block.reserve(bytes));
    struct Release {
        DeviceBuffer& b;
        ~Release() { b.release(); }
    } release{block};
    unsigned char* base = static_cast<unsigned char*>(block.ptr);
    uint32_t* assign = reinterpret_cast<uint32_t*>(base);
    uint32_t* prev = reinterpret_cast<uint32_t*>(base + o_prev);
    u64* gate_train = reinterpret_cast<u64*>(base + o_gate);
    u64* keys = reinterpret_cast<u64*>(base + o_keys);
    u64* sorted = reinterpret_cast<u64*>(base + o_sorted);
    u64* counter = reinterpret_cast<u64*>(base + o_cnt);
    float* cent = static_cast<float*>(centroids_.ptr);

    // the training gate; when the sample is every live row it is the live bitmap itself (null: every row)
    const u64* gate = v.live;
    std::vector<uint64_t> gate_host;
    if (!train_is_live) {
        gate_host.assign(words, 0ull);
        for (uint32_t r : train_rows) gate_host[r >> 6] |= 1ull << (r & 63);
        FSGPU_HIP(hipMemcpyAsync(gate_train, gate_host.data(), words * 8, hipMemcpyHostToDevice, stream));
        gate = gate_train;
    }
    // the initial centroids: the caller's, or the f32 widening of training row floor(c * T / nlist)
    std::vector<uint32_t> init_rows;
    if (init_centroids) {
        FSGPU_HIP(hipMemcpyAsync(cent, init_centroids, (size_t)nlist * dim * 4, hipMemcpyHostToDevice, stream));
    } else {
        const uint64_t T = train_rows.size();
        init_rows.resize(nlist);
        for (uint32_t c = 0; c < nlist; ++c) init_rows[c] = train_rows[(size_t)(((unsigned __int128)c * T) / nlist)];
        FSGPU_HIP(hipMemcpyAsync(base + o_init, init_rows.data(), (size_t)nlist * 4, hipMemcpyHostToDevice, stream));
        KnnStageArgs s{};
        s.slab = v.slab;
        s.row_stride = v.row_stride;
        s.dim = dim;
        s.slab_f32 = 0;
        s.row_base = v.row_base;
        s.src_local = reinterpret_cast<const uint32_t*>(base + o_init);
        s.n = nlist;
        s.queries = cent;
        s.src_out = reinterpret_cast<uint32_t*>(base + o_init_out);
        FSGPU_HIP(launch_knn_stage_rows(s, stream));
    }
    FSGPU_HIP(hipMemsetAsync(prev, 0xff, (size_t)n * 4, stream));
    FSGPU_HIP(hipMemsetAsync(counter, 0, 8, stream));
    FSGPU_HIP(hipStreamSynchronize(stream));   // (the host images above are done with)

    StageTimer timer{ev_begin_, ev_end_, stream};
    auto run_assign = [&](const u64* g, uint32_t* out) -> SearchError {
        FSGPU_HIP(timer.start());
        FSGPU_HIP(hipMemsetAsync(out, 0xff, (size_t)n * 4, stream));   // a row outside the gate: in no list
        IvfAssignArgs a{};
        a.slab = v.slab;
        a.row_stride = v.row_stride;
        a.dim = dim;
        a.hreduce = hreduce_;
        a.gate = g;
        a.centroids = cent;
        a.nlist = nlist;
        a.assign = out;
        for (uint32_t r0 = 0; r0 < n; r0 += kIvfLaunchRows) {
            a.row0 = r0;
            a.nrows = std::min<uint32_t>(kIvfLaunchRows, n - r0);
            FSGPU_HIP(launch_ivf_assign(a, stream));
        }
        FSGPU_HIP(timer.stop(&build_.assign_ms));
        return ok();
    };
    auto run_lists = [&](const uint32_t* from) -> SearchError {
        FSGPU_HIP(timer.start());
        FSGPU_HIP(launch_ivf_lists(from, n, nlist, keys, sorted, base + o_sort, sort_bytes, static_cast<u64*>(offsets_.ptr),
                                   static_cast<uint32_t*>(list_rows_.ptr), stream));
        FSGPU_HIP(timer.stop(&build_.lists_ms));
        return ok();
    };
    build_ = IvfBuildStats{};
    build_.rows_trained = train_rows.size();
    for (uint32_t it = 0; it < cfg_.iters; ++it) {
        FSGPU_TRY(run_assign(gate, assign));
        if (it + 1 == cfg_.iters) FSGPU_HIP(launch_ivf_count_changed(assign, prev, gate, n, counter, stream));
        FSGPU_TRY(run_lists(assign));
        FSGPU_HIP(timer.start());
        IvfUpdateArgs u{};
        u.slab = v.slab;
        u.row_stride = v.row_stride;
        u.dim = dim;
        u.list_rows = static_cast<const uint32_t*>(list_rows_.ptr);
        u.offsets = static_cast<const u64*>(offsets_.ptr);
        u.nlist = nlist;
        u.centroids = cent;
        FSGPU_HIP(launch_ivf_update(u, stream));
        FSGPU_HIP(timer.stop(&build_.update_ms));
        std::swap(assign, prev);
        build_.iterations += 1;
    }
    // all live rows against the final centroids
    FSGPU_TRY(run_assign(v.live, assign));
    FSGPU_TRY(run_lists(assign));
    offsets_host_.assign((size_t)nlist + 1, 0);
    uint64_t changed = 0;
    FSGPU_HIP(hipMemcpyAsync(offsets_host_.data(), offsets_.ptr, ((size_t)nlist + 1) * 8, hipMemcpyDeviceToHost, stream));
    FSGPU_HIP(hipMemcpyAsync(&changed, counter, 8, hipMemcpyDeviceToHost, stream));
    FSGPU_HIP(hipStreamSynchronize(stream));
    build_.rows_changed_last = changed;
    build_.smallest_list = ~0ull;
    for (uint32_t l = 0; l < nlist; ++l) {
        const uint64_t len = offsets_host_[l + 1] - offsets_host_[l];
        build_.empty_lists += len == 0;
        build_.largest_list = std::max(build_.largest_list, len);
        build_.smallest_list = std::min(build_.smallest_list, len);
    }
    return ok();
}

SearchError IvfIndex::check_handle() const {
    if (!index_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the handle was not initialised");
    if (index_->generation() != generation_ || index_->record_count() != nrows_)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the lists were made before the index was compacted or vacuumed: their row ids are stale");
    if (index_->hreduce != hreduce_)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the index's hreduce order has changed since the lists were made");
    return ok();
}

SearchError IvfIndex::check_call(uint32_t k, uint32_t nprobe) const {
    FSGPU_TRY(check_handle());
    if (k < 1 || k > kGatherMaxK || !filter_gather_supported(dim_, k))
        return make_error(FSGPU_ERR_INVALID_CONFIG, "1 <= k <= 256 does not hold, or the gather scan does not cover this k (k " + std::to_string(k) + ")");
    if (nprobe < 1 || nprobe > std::min(nlist_, kIvfMaxProbe))
        return make_error(FSGPU_ERR_INVALID_CONFIG, "1 <= nprobe <= min(nlist, 256) does not hold (nprobe " + std::to_string(nprobe) + ")");
    if ((uint64_t)nprobe * k > kIvfMergeMaxEntries)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "nprobe * k exceeds 16,384, the one-pass merge");
    return ok();
}

SearchError IvfIndex::centroids(float* out) {
    FSGPU_TRY(check_handle());
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_HIP(hipMemcpy(out, centroids_.ptr, (size_t)nlist_ * dim_ * 4, hipMemcpyDeviceToHost));
    return ok();
}

SearchError IvfIndex::lists(uint64_t* out_offsets, uint32_t* out_rows) {
    FSGPU_TRY(check_handle());
    FSGPU_HIP(hipSetDevice(device_));
    if (out_offsets) std::memcpy(out_offsets, offsets_host_.data(), ((size_t)nlist_ + 1) * 8);
    const uint64_t total = offsets_host_[nlist_];
    if (out_rows && total) FSGPU_HIP(hipMemcpy(out_rows, list_rows_.ptr, (size_t)total * 4, hipMemcpyDeviceToHost));
    return ok();
}

// ---- the int8 list filter ---------------------------------------------------------------------------------------------------
//
// The handle's copy: ordered[p] = filter_i8[list_rows[p]] list by list, a list's first row on a multiple of 16 rows, rows 64-byte
// pitched, everything else zero; beside it the scale word and the four statistics words the index's copy was built with and, for a
// rotated copy, the rotation and what it adds to the bound.  A query is prepared by the index's own kernel against exactly those.

SearchError IvfIndex::set_list_filter(uint32_t mode) {
    if (mode != FSGPU_IVF_LIST_FILTER_OFF && mode != FSGPU_IVF_LIST_FILTER_INT8)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "unknown list filter mode " + std::to_string(mode));
    FSGPU_TRY(check_handle());
    if (mode == FSGPU_IVF_LIST_FILTER_OFF || filter_built_) {
        filter_mode_ = mode;
        return ok();
    }
    VectorIndex::FilterCopyView fv;
    FSGPU_TRY(index_->ivf_filter_copy(&fv));
    FSGPU_HIP(hipSetDevice(device_));
    hipStream_t stream = index_->stream();
    for (hipEvent_t& e : fev_)
        if (!e) FSGPU_HIP(hipEventCreate(&e));
    const uint32_t pitch = (dim_ + kIvfFilterPitchAlign - 1) / kIvfFilterPitchAlign * kIvfFilterPitchAlign;
    uint64_t rows = 0;
    pad_row0_host_ = ivf_filter::pad_rows(nlist_, offsets_host_.data(), kIvfFilterRowTile, &rows);
    const size_t copy_bytes = (size_t)rows * pitch, o_pad = align256(copy_bytes);
    FSGPU_TRY(ordered_.reserve(o_pad + (size_t)nlist_ * 8));   // the copy | the lists' first rows
    FSGPU_TRY(filter_words_.reserve(32));
    u64* pad_dev = reinterpret_cast<u64*>(static_cast<unsigned char*>(ordered_.ptr) + o_pad);
    FSGPU_HIP(hipEventRecord(fev_[0], stream));
    if (copy_bytes) FSGPU_HIP(hipMemsetAsync(ordered_.ptr, 0, copy_bytes, stream));
    FSGPU_HIP(hipMemcpyAsync(pad_dev, pad_row0_host_.data(), (size_t)nlist_ * 8, hipMemcpyHostToDevice, stream));
    FSGPU_HIP(launch_ivf_filter_gather(fv.slab_i8, dim_, static_cast<const uint32_t*>(list_rows_.ptr), static_cast<const u64*>(offsets_.ptr), pad_dev,
                                       nlist_, offsets_host_[nlist_], pitch, static_cast<signed char*>(ordered_.ptr), stream));
    FSGPU_HIP(hipMemcpyAsync(filter_words_.ptr, fv.max_bits, 4, hipMemcpyDeviceToDevice, stream));
    FSGPU_HIP(hipMemcpyAsync(static_cast<unsigned char*>(filter_words_.ptr) + 16, fv.stats, 16, hipMemcpyDeviceToDevice, stream));
    if (fv.rotated) {
        FSGPU_TRY(filter_rot_mat_.reserve((size_t)dim_ * dim_ * 8));
        FSGPU_HIP(hipMemcpyAsync(filter_rot_mat_.ptr, fv.rot_mat, (size_t)dim_ * dim_ * 8, hipMemcpyDeviceToDevice, stream));
    }
    FSGPU_HIP(hipEventRecord(fev_[1], stream));
    FSGPU_HIP(hipStreamSynchronize(stream));
    float ms = 0.0f;
    FSGPU_HIP(hipEventElapsedTime(&ms, fev_[0], fev_[1]));
    filter_build_ms_ = ms;
    filter_rot_ = fv.rotated;
    filter_extra_coeff_ = fv.extra_coeff;
    filter_pitch_ = pitch;
    filter_rows_ = rows;
    filter_built_ = true;
    filter_mode_ = mode;
    return ok();
}

SearchError IvfIndex::filter_ordered_copy(signed char* out) {
    FSGPU_TRY(check_handle());
    if (!filter_built_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the handle has no ordered copy: the list filter was never enabled");
    FSGPU_HIP(hipSetDevice(device_));
    std::vector<signed char> phys((size_t)filter_rows_ * filter_pitch_);
    if (!phys.empty()) FSGPU_HIP(hipMemcpy(phys.data(), ordered_.ptr, phys.size(), hipMemcpyDeviceToHost));
    for (uint32_t l = 0; l < nlist_; ++l)
        for (uint64_t i = 0, len = offsets_host_[l + 1] - offsets_host_[l]; i < len; ++i)
            std::memcpy(out + (size_t)(offsets_host_[l] + i) * dim_, phys.data() + (size_t)(pad_row0_host_[l] + i) * filter_pitch_, dim_);
    return ok();
}

// codes [nq, dim] | delta [nq] (| the rotated queries) into fq_
SearchError IvfIndex::prepare_filter_queries(const float* q_dev, uint32_t nq, hipStream_t stream) {
    const size_t o_delta = align256((size_t)nq * dim_), o_rq = align256(o_delta + (size_t)nq * 4);
    FSGPU_TRY(fq_.reserve(o_rq + (filter_rot_ ? (size_t)nq * dim_ * 4 : 0)));
    unsigned char* base = static_cast<unsigned char*>(fq_.ptr);
    const unsigned int* words = static_cast<const unsigned int*>(filter_words_.ptr);
    const float* src = q_dev;
    if (filter_rot_) {
        float* rq = reinterpret_cast<float*>(base + o_rq);
        FSGPU_HIP(launch_rotate_rows_f32(q_dev, nq, dim_, dim_, static_cast<const double*>(filter_rot_mat_.ptr), rq, stream));
        src = rq;
    }
    FSGPU_HIP(launch_prepare_queries_i8_filter(src, nq, nq, dim_, dim_, words, words + 4, base, reinterpret_cast<float*>(base + o_delta), stream,
                                               nullptr, filter_rot_ ? filter_extra_coeff_ : 0.0));
    return ok();
}

void IvfIndex::filter_stats_begin(IvfFilterStats* f) const {
    *f = IvfFilterStats{};
    f->mode = filter_mode_;
    f->rotated = filter_rot_ ? 1u : 0u;
    f->slot_cap = kIvfFilterSlotCap;
    f->k_cap = kIvfFilterKCap;
    f->scratch_cap = scratch_entries_ ? scratch_entries_ : kIvfFilterScratchEntries;
    f->copy_bytes = filter_built_ ? filter_rows_ * filter_pitch_ : 0;
    f->build_ms = filter_build_ms_;
}

SearchError IvfIndex::search(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t* out_rows,
                             float* out_scores, uint32_t* out_counts, uint32_t* out_flags, bool on_device, IvfStats* stats, IvfFilterLab* lab) {
    FSGPU_TRY(check_call(k, nprobe));
    const uint32_t dim = dim_;
    if (query_len != dim)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "expected " + std::to_string(dim) + ", found " + std::to_string(query_len));
    VectorIndex::IvfSlabView v;
    FSGPU_TRY(index_->ivf_view(&v));
    IvfStats st;
    st.index_size = nrows_;
    st.dimension = dim;
    st.nlist = nlist_;
    st.nprobe = nprobe;
    st.k_requested = k;
    st.queries = nq;
    IvfFilterStats fs;
    filter_stats_begin(&fs);
    // the list filter takes the call when it is on and k is within its cap; the queries it cannot certify, the slots that overflow
    // and a call it does not take are scanned over their whole lists, as with the filter off
    const bool filt = filter_mode_ == FSGPU_IVF_LIST_FILTER_INT8 && filter_built_ && k <= kIvfFilterKCap;
    if (filter_mode_ == FSGPU_IVF_LIST_FILTER_INT8 && !filt && nq) fs.calls_above_k_cap = 1;
    if (lab && !filt) return make_error(FSGPU_ERR_INVALID_CONFIG, "the filter stage needs the list filter on and k <= 64");
    auto done = [&]() {
        last_ = st;
        flast_ = fs;
        if (stats) *stats = st;
        return ok();
    };
    if (nq == 0) return done();
    if ((uint64_t)nq * nprobe > 0x7fffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "nq * nprobe exceeds 2^31 - 1");
    FSGPU_HIP(hipSetDevice(device_));
    hipStream_t stream = index_->stream();
    const uint32_t pairs = nq * nprobe;

    // device block: counts | rows | scores (the head: what the host form copies up) | queries | coarse rows | scores | counts |
    // slot -> query | groups | per-query slots | the slots' queries | the slots' merged lists
    const size_t hits = (size_t)nq * k * 4;
    const size_t o_rows = align256((size_t)nq * 4), o_scores = align256(o_rows + (on_device ? 0 : hits)),
                 o_q = align256(o_scores + (on_device ? 0 : hits)), o_crows = align256(o_q + (on_device ? 0 : (size_t)nq * dim * 4)),
                 o_cscores = align256(o_crows + (size_t)pairs * 4), o_ccounts = align256(o_cscores + (size_t)pairs * 4),
                 o_cwork = align256(o_ccounts + (size_t)nq * 4), o_ccls = align256(o_cwork + (size_t)pairs * 8),
                 o_plan = align256(o_ccls + (size_t)nq);
    // the plan's image, offsets inside it: slot -> query [pairs] | groups [<= pairs] | per-query slots [pairs]
    const size_t p_groups = align256((size_t)pairs * 4), p_qslots = align256(p_groups + (size_t)pairs * sizeof(FilterGatherGroup)),
                 plan_bytes = align256(p_qslots + (size_t)pairs * 4);
    const size_t o_gq = align256(o_plan + plan_bytes), o_slot_lists = align256(o_gq + (size_t)pairs * dim * 4),
                 total = align256(o_slot_lists + (size_t)pairs * k * 8);
    FSGPU_TRY(ws_.reserve(total));
    const size_t p_delta = std::max(o_q, align256((size_t)pairs * 8));   // (the filter's bounds come up behind everything else)
    const size_t pin_need = p_delta + (filt ? align256((size_t)nq * 4) : 0);
    if (pin_bytes_ < pin_need) {
        if (pin_) (void)hipHostFree(pin_);
        pin_ = nullptr;
        pin_bytes_ = 0;
        FSGPU_HIP(hipHostMalloc(&pin_, pin_need, hipHostMallocDefault));
        pin_bytes_ = pin_need;
    }
    unsigned char* base = static_cast<unsigned char*>(ws_.ptr);
    unsigned char* pin = static_cast<unsigned char*>(pin_);
    if (!on_device) FSGPU_HIP(hipMemcpyAsync(base + o_q, queries, (size_t)nq * dim * 4, hipMemcpyHostToDevice, stream));
    const float* q_dev = on_device ? queries : reinterpret_cast<const float*>(base + o_q);
    uint32_t* c_rows = reinterpret_cast<uint32_t*>(base + o_crows);

    // (1) the coarse step: dot_product_f32_bytes_f32(centroid row, query), the nprobe best in the total order
    FSGPU_HIP(hipEventRecord(ev_begin_, stream));
    const float* delta_host = reinterpret_cast<const float*>(pin + p_delta);
    if (filt) {   // the filter's queries: codes and bounds, the bounds up with the coarse rows
        FSGPU_TRY(prepare_filter_queries(q_dev, nq, stream));
        FSGPU_HIP(hipMemcpyAsync(pin + p_delta, static_cast<unsigned char*>(fq_.ptr) + align256((size_t)nq * dim), (size_t)nq * 4,
                                 hipMemcpyDeviceToHost, stream));
    }
    const bool coarse_join = nq >= 16 && nprobe <= kKnnMaxM && dim <= kKnnUpdMaxDim;
    std::vector<uint32_t> probed_rows;
    const uint32_t* probed = nullptr;
    if (coarse_join) {
        // the batched search of so small an index is the exact F32 kernels, a few queries per pass: 11 ms of a 12 ms call at 1,024
        // queries x 1,024 lists.  The join's working table [nq, nprobe] comes back as packed (score, centroid) entries.
        u64* work = reinterpret_cast<u64*>(base + o_cwork);
        FSGPU_HIP(hipMemsetAsync(work, 0xff, (size_t)pairs * 8, stream));
        FSGPU_HIP(hipMemsetAsync(base + o_ccls, kKnnUpdClean, nq, stream));
        KnnUpdJoinArgs j{};
        j.slab = q_dev;
        j.row_stride = dim * 4;
        j.dim = dim;
        j.slab_f32 = 1;
        j.hreduce = hreduce_;
        j.row0 = 0;
        j.nrows = nq;
        j.m = nprobe;
        j.cls = base + o_ccls;
        j.work = work;
        j.added = static_cast<const float*>(centroids_.ptr);
        j.added_rows = static_cast<const uint32_t*>(coarse_ids_.ptr);
        j.n_added = nlist_;
        FSGPU_HIP(launch_knn_update_join(j, stream));
        FSGPU_HIP(hipMemcpyAsync(pin, work, (size_t)pairs * 8, hipMemcpyDeviceToHost, stream));
        FSGPU_HIP(hipStreamSynchronize(stream));
        probed_rows.resize(pairs);
        const u64* packed = reinterpret_cast<const u64*>(pin);
        for (uint32_t i = 0; i < pairs; ++i) probed_rows[i] = (uint32_t)packed[i];   // (an empty slot, which nprobe <= nlist rules out, fails the plan's range check)
        probed = probed_rows.data();
    } else {
        coarse_.hreduce = hreduce_;
        uint32_t coarse_fallbacks = 0;
        FSGPU_TRY(coarse_.search_top_k_batched_device(q_dev, nq, dim, nprobe, nullptr, c_rows, reinterpret_cast<float*>(base + o_cscores),
                                                      reinterpret_cast<uint32_t*>(base + o_ccounts), stream, &coarse_fallbacks));
        FSGPU_HIP(hipSetDevice(device_));
        FSGPU_HIP(hipMemcpyAsync(pin, c_rows, (size_t)pairs * 4, hipMemcpyDeviceToHost, stream));
        FSGPU_HIP(hipStreamSynchronize(stream));
        probed = reinterpret_cast<const uint32_t*>(pin);
    }
    st.launches += 1;

    // (2) the plan: a counting sort of the pairs by list (queries ascending inside a list)
    std::vector<uint32_t> head((size_t)nlist_ + 1, 0u);
    for (uint32_t i = 0; i < pairs; ++i) {
        if (probed[i] >= nlist_) return make_error(FSGPU_ERR_DEVICE, "the coarse search returned a centroid outside the matrix");
        ++head[probed[i] + 1];
    }
    uint32_t ngroups = 0;
    for (uint32_t l = 0; l < nlist_; ++l) {
        if (head[l + 1] && offsets_host_[l + 1] > offsets_host_[l]) ++ngroups;
        head[l + 1] += head[l];
    }
    std::vector<uint32_t> by_list(pairs);
    {
        std::vector<uint32_t> fill(head.begin(), head.end() - 1);
        for (uint32_t i = 0; i < pairs; ++i) by_list[fill[probed[i]]++] = i / nprobe;
    }
    plan_host_.assign(plan_bytes, 0);
    uint32_t* slot_query = reinterpret_cast<uint32_t*>(plan_host_.data());
    FilterGatherGroup* groups = reinterpret_cast<FilterGatherGroup*>(plan_host_.data() + p_groups);
    uint32_t* qslots = reinterpret_cast<uint32_t*>(plan_host_.data() + p_qslots);
    std::vector<uint32_t> qfill(nq, 0u);
    // blocks per probed list: over all groups about four per CU, few enough that a slot's block lists fit merge_topk's one-pass
    // form, never more than the list has tiles
    const uint32_t by_device = std::min<uint32_t>(1024, std::max<uint32_t>(1, (uint32_t)(4 * v.num_cus) / std::max<uint32_t>(ngroups, 1)));
    const uint32_t cap = std::max<uint32_t>(1, std::min<uint32_t>(by_device, 16384 / k));
    uint32_t slots = 0, grid_x = 0, g = 0;
    const uint32_t* list_rows = static_cast<const uint32_t*>(list_rows_.ptr);
    for (uint32_t l = 0; l < nlist_; ++l) {
        const uint32_t cnt = head[l + 1] - head[l];
        if (!cnt) continue;
        const uint64_t len = offsets_host_[l + 1] - offsets_host_[l];
        st.lists_probed += cnt;
        st.rows_scored += len * cnt;
        for (uint32_t i = 0; i < cnt; ++i) {
            const uint32_t q = by_list[head[l] + i];
            qslots[(size_t)q * nprobe + qfill[q]++] = len ? slots + i : kIvfNoSlot;
            if (len) slot_query[slots + i] = q;
        }
        if (!len) continue;   // an empty list gets no group
        FilterGatherGroup& gd = groups[g++];
        gd.rows = list_rows + offsets_host_[l];
        gd.n = (uint32_t)len;
        gd.q0 = slots;
        gd.nq = cnt;
        gd.nblocks = std::min<uint32_t>((gd.n + kGatherTileRows - 1) / kGatherTileRows, cap);
        grid_x = std::max(grid_x, gd.nblocks);
        slots += cnt;
    }
    FSGPU_HIP(hipMemcpyAsync(base + o_plan, plan_host_.data(), plan_bytes, hipMemcpyHostToDevice, stream));

    // (2f) the list filter: every probed list scored once on the matrix cores for all its member queries, per slot the rows that can
    // still reach its exact top k, and the SECOND plan: one single-member group per filtered slot over its candidates, today's groups
    // for the members that overflowed, are not certified or did not fit the scratch
    if (fs.calls_above_k_cap) fs.rows_rescored = st.rows_scored;   // every exact dot was made
    if (filt) {
        uint32_t certified = 0;
        for (uint32_t q = 0; q < nq; ++q) certified += delta_host[q] >= 0.0f;
        fs.queries_filtered = certified;
        fs.queries_uncertified = nq - certified;
        fs.rows_rescored = st.rows_scored;
        if (lab) lab->delta.assign(delta_host, delta_host + nq);
        if (certified && slots) {
            const ivf_filter::Caps caps{fs.scratch_cap, kIvfFilterTileQueries, kIvfFilterRowTile, kIvfFilterItemRows, kIvfFilterSlotCap};
            ivf_filter::ScorePlan sp = ivf_filter::score_plan(nlist_, offsets_host_.data(), head.data(), pad_row0_host_.data(), caps);
            if (sp.slots != slots) return make_error(FSGPU_ERR_DEVICE, "the filter's plan disagrees with the search's about the slots");
            const uint32_t ntiles = (uint32_t)sp.tiles.size() - 1;
            if (lab && (sp.ranges.size() != 1 || sp.ranges[0].ntiles != ntiles))
                return make_error(FSGPU_ERR_INVALID_CONFIG, "the filter stage needs a call whose scores fit the scratch at once");
            // device: tiles | slot -> tile, and per slot t | m | count | flag | candidates
            const size_t f_slot_tile = align256(sp.tiles.size() * sizeof(IvfFilterTile));
            FSGPU_TRY(fplan_.reserve(f_slot_tile + (size_t)slots * 4));
            unsigned char* fp = static_cast<unsigned char*>(fplan_.ptr);
            FSGPU_HIP(hipMemcpyAsync(fp, sp.tiles.data(), sp.tiles.size() * sizeof(IvfFilterTile), hipMemcpyHostToDevice, stream));
            FSGPU_HIP(hipMemcpyAsync(fp + f_slot_tile, sp.slot_tile.data(), (size_t)slots * 4, hipMemcpyHostToDevice, stream));
            uint64_t entries = 0;
            for (const ivf_filter::Range& r : sp.ranges) entries = std::max(entries, r.entries);
            const size_t s_m = align256((size_t)slots * 4), s_count = align256(s_m + (size_t)slots * 8), s_cand = align256(s_count + (size_t)slots * 8);
            int32_t* scores_dev = nullptr;
            int32_t* t_dev = nullptr;
            long long* m_dev = nullptr;
            uint32_t *count_dev = nullptr, *flag_dev = nullptr, *cand_dev = nullptr;
            if (lab) {
                scores_dev = static_cast<int32_t*>(lab->alloc(IvfFilterLab::kScores, (size_t)entries * 4));
                t_dev = static_cast<int32_t*>(lab->alloc(IvfFilterLab::kT, (size_t)slots * 4));
                m_dev = static_cast<long long*>(lab->alloc(IvfFilterLab::kM, (size_t)slots * 8));
                count_dev = static_cast<uint32_t*>(lab->alloc(IvfFilterLab::kCount, (size_t)slots * 4));
                flag_dev = static_cast<uint32_t*>(lab->alloc(IvfFilterLab::kFlag, (size_t)slots * 4));
                cand_dev = static_cast<uint32_t*>(lab->alloc(IvfFilterLab::kCand, (size_t)slots * kIvfFilterSlotCap * 4));
                if (!scores_dev || !t_dev || !m_dev || !count_dev || !flag_dev || !cand_dev)
                    return make_error(FSGPU_ERR_DEVICE, "the filter stage's outputs could not be allocated");
            } else {
                FSGPU_TRY(fscratch_.reserve(std::max<size_t>((size_t)entries * 4, 256)));
                FSGPU_TRY(fslot_.reserve(s_cand + (size_t)slots * kIvfFilterSlotCap * 4));
                unsigned char* sb = static_cast<unsigned char*>(fslot_.ptr);
                scores_dev = static_cast<int32_t*>(fscratch_.ptr);
                t_dev = reinterpret_cast<int32_t*>(sb);
                m_dev = reinterpret_cast<long long*>(sb + s_m);
                count_dev = reinterpret_cast<uint32_t*>(sb + s_count);   // counts | flags: one copy brings both up
                flag_dev = count_dev + slots;
                cand_dev = reinterpret_cast<uint32_t*>(sb + s_cand);
            }
            // a slot of a tile above the scratch is in no range: nothing writes its count and flag but this
            FSGPU_HIP(hipMemsetAsync(count_dev, 0, (size_t)slots * 4, stream));
            FSGPU_HIP(hipMemsetAsync(flag_dev, 0, (size_t)slots * 4, stream));
            IvfFilterScoreArgs sa{};
            sa.ordered = static_cast<const signed char*>(ordered_.ptr);
            sa.pitch = filter_pitch_;
            sa.codes = static_cast<const signed char*>(fq_.ptr);
            sa.dim = dim;
            sa.slot_query = reinterpret_cast<const uint32_t*>(base + o_plan);
            sa.list_rows = list_rows;
            sa.live = v.live;   // as it is NOW
            sa.tiles = reinterpret_cast<const IvfFilterTile*>(fp);
            sa.scores = scores_dev;
            IvfFilterSelectArgs se{};
            se.scores = scores_dev;
            se.tiles = sa.tiles;
            se.slot_tile = reinterpret_cast<const uint32_t*>(fp + f_slot_tile);
            se.slot_query = sa.slot_query;
            se.delta = reinterpret_cast<const float*>(static_cast<unsigned char*>(fq_.ptr) + align256((size_t)nq * dim));
            se.list_rows = list_rows;
            se.k = k;
            se.out_t = t_dev;
            se.out_m = m_dev;
            se.out_count = count_dev;
            se.out_flag = flag_dev;
            se.cand = cand_dev;
            for (const ivf_filter::Range& r : sp.ranges) {
                sa.tile_first = r.tile_first;
                sa.ntiles = r.ntiles;
                sa.item_first = r.item_first;
                se.slot_first = r.slot_first;
                FSGPU_HIP(hipEventRecord(fev_[0], stream));
                FSGPU_HIP(launch_ivf_filter_score(sa, r.nitems, stream));
                FSGPU_HIP(hipEventRecord(fev_[1], stream));
                FSGPU_HIP(launch_ivf_filter_select(se, r.nslots, stream));
                FSGPU_HIP(hipEventRecord(fev_[2], stream));
                FSGPU_HIP(hipEventSynchronize(fev_[2]));   // (the next range reuses the scratch and the events)
                float ms_score = 0.0f, ms_select = 0.0f;
                FSGPU_HIP(hipEventElapsedTime(&ms_score, fev_[0], fev_[1]));
                FSGPU_HIP(hipEventElapsedTime(&ms_select, fev_[1], fev_[2]));
                fs.filter_ms += ms_score;
                fs.select_ms += ms_select;
                st.launches += 2;
                for (uint32_t t = r.tile_first; t < r.tile_first + r.ntiles; ++t) fs.rows_streamed += sp.tiles[t].len;
            }
            fs.scratch_ranges = sp.ranges.size();
            uint32_t* cf = reinterpret_cast<uint32_t*>(pin);   // (2 x slots words <= pairs x 8 bytes; the coarse rows are done with)
            if (lab) {
                FSGPU_HIP(hipMemcpyAsync(cf, count_dev, (size_t)slots * 4, hipMemcpyDeviceToHost, stream));
                FSGPU_HIP(hipMemcpyAsync(cf + slots, flag_dev, (size_t)slots * 4, hipMemcpyDeviceToHost, stream));
            } else {
                FSGPU_HIP(hipMemcpyAsync(cf, count_dev, (size_t)slots * 8, hipMemcpyDeviceToHost, stream));
            }
            FSGPU_HIP(hipStreamSynchronize(stream));
            std::vector<uint32_t> counts2(cf, cf + slots), flags2(cf + slots, cf + 2 * (size_t)slots);
            for (uint32_t t = 0; t < ntiles; ++t)
                if (sp.above[t])
                    for (uint32_t j = 0; j < sp.tiles[t].nmem; ++j) flags2[sp.tiles[t].slot0 + j] = kIvfFilterFlagAboveScratch;
            for (uint32_t s = 0; s < slots; ++s) {
                if (flags2[s] & kIvfFilterFlagAboveScratch) {
                    fs.slots_above_scratch += delta_host[slot_query[s]] >= 0.0f;
                    continue;
                }
                if (flags2[s] & kIvfFilterFlagUncertified) continue;
                fs.slots_filtered += 1;
                fs.slots_overflowed += (flags2[s] & kIvfFilterFlagOverflow) != 0;
                fs.rows_filtered += sp.tiles[sp.slot_tile[s]].len;
            }
            const ivf_filter::ScanPlan scan = ivf_filter::scan_plan(nlist_, offsets_host_.data(), head.data(), counts2.data(), flags2.data(), k,
                                                                    (uint32_t)v.num_cus, kGatherTileRows, caps);
            fs.rows_rescored = scan.rows_rescored;
            ngroups = (uint32_t)scan.groups.size();
            grid_x = scan.grid_x;
            for (uint32_t i = 0; i < ngroups; ++i) {   // (the first plan's image has been uploaded: the stream was synchronised above)
                const ivf_filter::Group& sg = scan.groups[i];
                FilterGatherGroup& gd = groups[i];
                gd.rows = (sg.from_cand ? cand_dev : list_rows) + sg.rows_off;
                gd.n = sg.n;
                gd.q0 = sg.q0;
                gd.nq = sg.nq;
                gd.nblocks = sg.nblocks;
            }
            FSGPU_HIP(hipMemcpyAsync(base + o_plan + p_groups, plan_host_.data() + p_groups, (size_t)ngroups * sizeof(FilterGatherGroup),
                                     hipMemcpyHostToDevice, stream));
            if (lab) {
                lab->tiles = sp.tiles;
                lab->slot_tile = sp.slot_tile;
                lab->slot_query.assign(slot_query, slot_query + slots);
                lab->slot_list.resize(slots);
                for (uint32_t l = 0, s = 0; l < nlist_; ++l)
                    if (offsets_host_[l + 1] > offsets_host_[l])
                        for (uint32_t i = head[l]; i < head[l + 1]; ++i) lab->slot_list[s++] = l;
                lab->entries = entries;
                lab->ran = true;
            }
        }
    }

    // (3) the probed lists: one segmented gather scan, its blocks' lists merged per slot
    const uint32_t list_stride = k <= 64 ? 64 : k;
    IvfMergeArgs m{};
    m.slot_lists = reinterpret_cast<const u64*>(base + o_slot_lists);
    m.slot_stride = k;
    if (filt) FSGPU_HIP(hipEventRecord(fev_[0], stream));   // rescore_ms: the exact scan and its merge
    if (slots) {
        FSGPU_TRY(ws_lists_.reserve((size_t)slots * grid_x * list_stride * 8));
        float* gq = reinterpret_cast<float*>(base + o_gq);
        FSGPU_HIP(launch_gather_queries(q_dev, reinterpret_cast<const uint32_t*>(base + o_plan), slots, dim, dim, gq, stream));
        FilterGatherArgs a;
        a.slab = v.slab;
        a.live = v.live;   // as it is NOW: deletes made after the build are honoured
        a.queries = gq;
        a.partial = static_cast<u64*>(ws_lists_.ptr);
        a.list_stride = list_stride;
        a.nrows = v.nrows;
        a.dim = dim;
        a.k = k;
        a.row_base = v.row_base;
        a.row_stride = v.row_stride;
        a.hreduce = hreduce_;
        constexpr uint32_t kMaxGridY = 65535;
        const FilterGatherGroup* groups_dev = reinterpret_cast<const FilterGatherGroup*>(base + o_plan + p_groups);
        for (uint32_t g0 = 0; g0 < ngroups; g0 += kMaxGridY) {
            a.groups = groups_dev + g0;
            FSGPU_HIP(launch_filter_gather_scan(a, std::min(ngroups - g0, kMaxGridY), grid_x, stream));
            st.launches += 1;
        }
        if (grid_x == 1) {   // one block per list: its list IS the slot's
            m.slot_lists = a.partial;
            m.slot_stride = list_stride;
        } else {
            MergeArgs mm;
            mm.lists = a.partial;
            mm.q_stride = (uint64_t)grid_x * list_stride;
            mm.l_stride = list_stride;
            mm.nlists = grid_x;
            mm.list_len = k;
            mm.k = k;
            mm.out_stride = k;
            mm.out_rows = nullptr;
            mm.out_scores = nullptr;
            mm.out_counts = nullptr;
            mm.out_packed = reinterpret_cast<u64*>(base + o_slot_lists);
            FSGPU_HIP(launch_merge_topk(mm, (int)slots, stream));
        }
    }
    if (filt) FSGPU_HIP(hipEventRecord(fev_[1], stream));
    // (4) the per-query merge
    m.qslots = reinterpret_cast<const uint32_t*>(base + o_plan + p_qslots);
    m.nprobe = nprobe;
    m.k = k;
    m.out_rows = on_device ? out_rows : reinterpret_cast<uint32_t*>(base + o_rows);
    m.out_scores = on_device ? out_scores : reinterpret_cast<float*>(base + o_scores);
    m.out_counts = on_device ? out_counts : reinterpret_cast<uint32_t*>(base);
    FSGPU_HIP(launch_ivf_merge(m, nq, stream));
    FSGPU_HIP(hipEventRecord(ev_end_, stream));
    // (5) counts (and, host form, hits) up in one copy
    if (on_device) FSGPU_HIP(hipMemcpyAsync(pin, out_counts, (size_t)nq * 4, hipMemcpyDeviceToHost, stream));
    else FSGPU_HIP(hipMemcpyAsync(pin, base, o_q, hipMemcpyDeviceToHost, stream));
    FSGPU_HIP(hipStreamSynchronize(stream));
    std::vector<uint32_t> counts(reinterpret_cast<const uint32_t*>(pin), reinterpret_cast<const uint32_t*>(pin) + nq), flags(nq, 0u);
    uint32_t* rows = reinterpret_cast<uint32_t*>(pin + o_rows);   // (host form)
    float* scores = reinterpret_cast<float*>(pin + o_scores);
    float ms = 0.0f;
    FSGPU_HIP(hipEventElapsedTime(&ms, ev_begin_, ev_end_));
    st.device_ms = ms;
    if (filt) {
        FSGPU_HIP(hipEventElapsedTime(&ms, fev_[0], fev_[1]));
        fs.rescore_ms = ms;
    }

    // the fallback (hnsw.rs:1150-1190): count < min(k, live rows) -> the exact search answers
    std::vector<uint32_t> under;
    if (std::any_of(counts.begin(), counts.end(), [&](uint32_t c) { return c < k; })) {
        FSGPU_TRY(index_->fetch_live_host());
        const uint64_t need = std::min<uint64_t>(k, index_->live_count());
        for (uint32_t q = 0; q < nq; ++q)
            if (counts[q] < need) {
                flags[q] = counts[q] == 0 ? (uint32_t)FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS : (uint32_t)FSGPU_ANN_UNDERFILLED;
                under.push_back(q);
            }
    }
    if (!under.empty()) {
        const uint32_t nu = (uint32_t)under.size();
        std::vector<float> uq((size_t)nu * dim), us((size_t)nu * k);
        std::vector<uint32_t> ur((size_t)nu * k), uc(nu);
        for (uint32_t i = 0; i < nu; ++i) {
            if (on_device) FSGPU_HIP(hipMemcpy(uq.data() + (size_t)i * dim, queries + (size_t)under[i] * dim, (size_t)dim * 4, hipMemcpyDeviceToHost));
            else std::memcpy(uq.data() + (size_t)i * dim, queries + (size_t)under[i] * dim, (size_t)dim * 4);
        }
        FSGPU_TRY(index_->search_top_k_batched(uq.data(), nu, dim, k, nullptr, ur.data(), us.data(), uc.data(), nullptr));
        for (uint32_t i = 0; i < nu; ++i) {
            const uint32_t q = under[i];
            counts[q] = uc[i];
            if (on_device) {
                FSGPU_HIP(hipMemcpy(out_rows + (size_t)q * k, ur.data() + (size_t)i * k, (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_scores + (size_t)q * k, us.data() + (size_t)i * k, (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_counts + q, &uc[i], 4, hipMemcpyHostToDevice));
            } else {
                std::memcpy(rows + (size_t)q * k, ur.data() + (size_t)i * k, (size_t)k * 4);
                std::memcpy(scores + (size_t)q * k, us.data() + (size_t)i * k, (size_t)k * 4);
            }
        }
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (flags[q] == FSGPU_ANN_UNDERFILLED) st.underfilled += 1;
        else if (flags[q] == FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS) st.empty_despite_indexed_points += 1;
        else st.approximate += 1;
    }
    if (on_device) {
        if (out_flags) FSGPU_HIP(hipMemcpy(out_flags, flags.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
    } else {
        std::memcpy(out_rows, rows, hits);
        std::memcpy(out_scores, scores, hits);
        std::memcpy(out_counts, counts.data(), (size_t)nq * 4);
        if (out_flags) std::memcpy(out_flags, flags.data(), (size_t)nq * 4);
    }
    return done();
}

SearchError IvfIndex::certify_nprobe(const float* queries, uint32_t nq, const uint32_t* candidates, uint32_t n_candidates, uint32_t k, double target,
                                     double alpha, CertifiedEf* chosen, CertifiedEf* sweep, uint32_t* n_swept) {
    if (n_candidates == 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "no candidate nprobe");
    std::vector<uint32_t> probes(candidates, candidates + n_candidates);
    std::sort(probes.begin(), probes.end());
    probes.erase(std::unique(probes.begin(), probes.end()), probes.end());
    for (uint32_t p : probes) FSGPU_TRY(check_call(k, p));
    const uint32_t dim = dim_;
    // the exact top-k is independent of nprobe: once per query
    std::vector<uint32_t> erows((size_t)nq * k), ecounts(nq, 0u), arows((size_t)nq * k), acounts(nq), aflags(nq);
    std::vector<float> escores((size_t)nq * k), ascores((size_t)nq * k);
    if (nq) FSGPU_TRY(index_->search_top_k_batched(queries, nq, dim, k, nullptr, erows.data(), escores.data(), ecounts.data(), nullptr));
    IvfStats sum;
    IvfFilterStats fsum;
    filter_stats_begin(&fsum);
    std::vector<double> recalls(nq);
    bool have_best = false;
    CertifiedEf best;
    uint32_t swept = 0;
    for (uint32_t p : probes) {
        IvfStats st;
        FSGPU_TRY(search(queries, nq, dim, k, p, arows.data(), ascores.data(), acounts.data(), aflags.data(), false, &st));
        sum.index_size = st.index_size;
        sum.dimension = st.dimension;
        sum.nlist = st.nlist;
        sum.k_requested = k;
        sum.nprobe = std::max(sum.nprobe, p);
        sum.launches += st.launches;
        sum.queries += st.queries;
        sum.approximate += st.approximate;
        sum.underfilled += st.underfilled;
        sum.empty_despite_indexed_points += st.empty_despite_indexed_points;
        sum.lists_probed += st.lists_probed;
        sum.rows_scored += st.rows_scored;
        sum.device_ms += st.device_ms;
        fsum.queries_filtered += flast_.queries_filtered;
        fsum.queries_uncertified += flast_.queries_uncertified;
        fsum.calls_above_k_cap += flast_.calls_above_k_cap;
        fsum.slots_filtered += flast_.slots_filtered;
        fsum.slots_overflowed += flast_.slots_overflowed;
        fsum.slots_above_scratch += flast_.slots_above_scratch;
        fsum.scratch_ranges += flast_.scratch_ranges;
        fsum.rows_filtered += flast_.rows_filtered;
        fsum.rows_rescored += flast_.rows_rescored;
        fsum.rows_streamed += flast_.rows_streamed;
        fsum.filter_ms += flast_.filter_ms;
        fsum.select_ms += flast_.select_ms;
        fsum.rescore_ms += flast_.rescore_ms;
        for (uint32_t q = 0; q < nq; ++q)
            recalls[q] = aflags[q] ? 0.0
                                   : recall_at_k_of_rows(arows.data() + (size_t)q * k, acounts[q], erows.data() + (size_t)q * k, ecounts[q]);
        CertifiedEf c;
        c.ef_search = p;
        c.certified_recall = conformal_recall_lower_bound(recalls.data(), nq, alpha);
        c.meets_target = c.certified_recall >= target;
        sweep[swept++] = c;
        if (c.meets_target) {
            best = c;
            have_best = true;
            break;
        }
        if (!have_best || c.certified_recall > best.certified_recall) {
            best = c;
            have_best = true;
        }
    }
    last_ = sum;
    flast_ = fsum;
    *chosen = best;
    *n_swept = swept;
    return ok();
}

}  // namespace fsgpu

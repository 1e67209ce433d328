// ivf_index.hpp — the host side of the inverted-file index (include/fsgpu.h, "IVF index"; ivf_kernels.hip): spherical
// Lloyd k-means over an index's rows trained on its device, the inverted lists, the probed-list search — a coarse batched search of
// the centroid matrix, a host plan, ONE segmented gather scan (filter_gather_kernels.hip) and its merges — with the reference's
// underfill fallback (hnsw.rs:299-309), and certify_nprobe: ann_index.cpp's certify_ef with nprobe in the place of ef.
#pragma once

#include <cstdint>
#include <functional>
#include <vector>

#include "ann_index.hpp"
#include "ivf_filter_plan.hpp"
#include "vector_index.hpp"

namespace fsgpu {

struct IvfConfig {
    uint32_t iters = 8;      // Lloyd iterations, 0 .. kIvfMaxIters
    uint64_t n_train = 0;    // strided training sample; 0 or >= record_count: every live row
};

struct IvfBuildStats {   // field for field fsgpu_ivf_build_stats
    uint32_t iterations = 0;
    uint64_t rows_trained = 0, rows_changed_last = 0, empty_lists = 0, largest_list = 0, smallest_list = 0;
    double assign_ms = 0.0, update_ms = 0.0, lists_ms = 0.0;
};

struct IvfStats {   // field for field fsgpu_ivf_stats
    uint64_t index_size = 0;
    uint32_t dimension = 0, nlist = 0, nprobe = 0, k_requested = 0, launches = 0;
    uint64_t queries = 0, approximate = 0, underfilled = 0, empty_despite_indexed_points = 0, lists_probed = 0, rows_scored = 0;
    double device_ms = 0.0;
};

struct IvfFilterStats {   // field for field fsgpu_ivf_filter_stats
    uint32_t mode = 0, rotated = 0, slot_cap = 0, k_cap = 0;
    uint64_t scratch_cap = 0, copy_bytes = 0;
    double build_ms = 0.0;
    uint64_t queries_filtered = 0, queries_uncertified = 0, calls_above_k_cap = 0, slots_filtered = 0, slots_overflowed = 0,
             slots_above_scratch = 0, scratch_ranges = 0, rows_filtered = 0, rows_rescored = 0, rows_streamed = 0;
    double filter_ms = 0.0, select_ms = 0.0, rescore_ms = 0.0;
};

// What fsgpu_lab_ivf_filter_stage asks of a search: the filter's device outputs come from `alloc` (guarded buffers of the lab harness)
// instead of the handle's workspaces, and the host tables of the call are left here.
struct IvfFilterLab {
    enum Which { kScores = 0, kT, kM, kCount, kFlag, kCand };
    std::function<void*(Which, size_t bytes)> alloc;   // null return: the allocation failed (the harness keeps the error)
    std::vector<IvfFilterTile> tiles;                  // [ntiles + 1]
    std::vector<uint32_t> slot_query, slot_list, slot_tile;
    std::vector<float> delta;                          // [nq]
    uint64_t entries = 0;                              // of the scores
    bool ran = false;                                  // the filter stage ran (some query was certified, k <= the cap)
};

class IvfIndex {
  public:
    ~IvfIndex();
    IvfIndex() = default;
    IvfIndex(const IvfIndex&) = delete;
    IvfIndex& operator=(const IvfIndex&) = delete;

    // trains and builds; every limit that does not depend on a call (include/fsgpu.h) is checked here, before anything is allocated.
    // init_centroids: host [nlist, dim] or null (the strided rows).  Blocks.  The caller holds the index's mutex.
    SearchError init(VectorIndex* index, uint32_t nlist, const float* init_centroids, const IvfConfig& config);
    uint64_t record_count() const { return nrows_; }
    uint32_t nlist() const { return nlist_; }
    int device() const { return device_; }
    const IvfBuildStats& build_stats() const { return build_; }
    SearchError centroids(float* out);                          // host [nlist, dim]
    SearchError lists(uint64_t* out_offsets, uint32_t* out_rows);   // host [nlist + 1], [out_offsets[nlist]] local rows
    // on_device: queries and the four outputs are device pointers (out_flags may be null either way).  Blocks.
    SearchError search(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t* out_rows, float* out_scores,
                       uint32_t* out_counts, uint32_t* out_flags, bool on_device, IvfStats* stats, IvfFilterLab* lab = nullptr);
    // The int8 list filter.  mode 1 builds the handle's cluster-ordered int8 copy on first use (blocks; builds the
    // index's filter copy if need be); an unknown mode is refused before anything is built.
    SearchError set_list_filter(uint32_t mode);
    uint32_t list_filter() const { return filter_mode_; }
    IvfFilterStats last_filter_stats() const {   // the last call's figures beside the handle's mode, copy and caps as they stand
        IvfFilterStats now, f = flast_;
        filter_stats_begin(&now);
        f.mode = now.mode, f.rotated = now.rotated, f.slot_cap = now.slot_cap, f.k_cap = now.k_cap, f.scratch_cap = now.scratch_cap;
        f.copy_bytes = now.copy_bytes, f.build_ms = now.build_ms;
        return f;
    }
    SearchError filter_ordered_copy(signed char* out);          // host [offsets[nlist], dim]: the logical ordered copy
    void set_filter_scratch_entries(uint64_t entries) { scratch_entries_ = entries; }   // (lab) 0: the default
    // sweep holds n_probes entries; CertifiedEf::ef_search carries nprobe
    SearchError certify_nprobe(const float* queries, uint32_t nq, const uint32_t* candidates, uint32_t n_candidates, uint32_t k, double target,
                               double alpha, CertifiedEf* chosen, CertifiedEf* sweep, uint32_t* n_swept);
    const IvfStats& last_stats() const { return last_; }

  private:
    SearchError check_handle() const;
    SearchError check_call(uint32_t k, uint32_t nprobe) const;
    SearchError train(const VectorIndex::IvfSlabView& v, const float* init_centroids, const std::vector<uint32_t>& train_rows, bool train_is_live);
    VectorIndex* index_ = nullptr;
    VectorIndex coarse_;   // an F32 index over the centroid matrix, in the parent's hreduce order: the coarse quantiser at query time
    int device_ = -1;      // the index's device, kept here: the destructor frees device memory and must not need the index for it
    uint64_t nrows_ = 0, generation_ = 0;
    int32_t hreduce_ = 0;
    uint32_t nlist_ = 0, dim_ = 0;
    IvfConfig cfg_;
    IvfBuildStats build_;
    DeviceBuffer centroids_, offsets_, list_rows_, ws_, ws_lists_;
    DeviceBuffer coarse_ids_;   // 0 .. nlist - 1: the centroids' ids, as the coarse join wants them beside the streamed block
    std::vector<uint64_t> offsets_host_;   // [nlist + 1]: the plan reads list lengths here
    std::vector<unsigned char> plan_host_; // the host image of a call's plan (alive until the call has synchronised)
    void* pin_ = nullptr;                  // pinned block the coarse rows, and the counts and hits of a call, come up through
    size_t pin_bytes_ = 0;
    hipEvent_t ev_begin_ = nullptr, ev_end_ = nullptr;
    IvfStats last_;
    // the int8 list filter: the ordered copy and what it was built from — never the index's own buffers, which the index may rebuild
    // (adopt_global_quant_max) or drop without a generation change of its own making
    SearchError prepare_filter_queries(const float* q_dev, uint32_t nq, hipStream_t stream);
    void filter_stats_begin(IvfFilterStats* f) const;
    uint32_t filter_mode_ = 0;
    bool filter_built_ = false, filter_rot_ = false;
    double filter_extra_coeff_ = 0.0, filter_build_ms_ = 0.0;
    uint32_t filter_pitch_ = 0;
    uint64_t filter_rows_ = 0, scratch_entries_ = 0;
    std::vector<uint64_t> pad_row0_host_;   // [nlist]
    DeviceBuffer ordered_, filter_words_ /* scale word | statistics */, filter_rot_mat_, fq_, fscratch_, fslot_, fplan_;
    hipEvent_t fev_[3] = {nullptr, nullptr, nullptr};
    IvfFilterStats flast_;
};

}  // namespace fsgpu

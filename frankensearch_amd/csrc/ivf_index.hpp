// ivf_index.hpp — the host side of the inverted-file index (include/fsgpu.h, "IVF index"; ivf_kernels.hip): spherical
// Lloyd k-means over an index's rows trained on its device, the inverted lists, the probed-list search — a coarse batched search of
// the centroid matrix, a host plan, ONE segmented gather scan (filter_gather_kernels.hip) and its merges — with the reference's
// underfill fallback (hnsw.rs:299-309), and certify_nprobe: ann_index.cpp's certify_ef with nprobe in the place of ef.
#pragma once

#include <cstdint>
#include <vector>

#include "ann_index.hpp"
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
                       uint32_t* out_counts, uint32_t* out_flags, bool on_device, IvfStats* stats);
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
};

}  // namespace fsgpu

// ann_index.hpp — the host side of the graph ANN search (include/fsgpu.h, "graph ANN search"; ann_kernels.hip):
// a k-NN table resident on an index's device, the beam search over it with the reference's underfill fallback and stats
// (HnswIndex::knn_search_with_stats, crates/frankensearch-index/src/hnsw.rs:842-1330), certify_ef_search (hnsw.rs:1354-1386), and
// the recall certificates (recall_certificate.rs:50-292) as plain host functions.
#pragma once

#include <cstdint>
#include <vector>

#include "vector_index.hpp"

namespace fsgpu {

struct AnnConfig {
    uint32_t n_entry = 1024;   // clamped to record_count
    uint32_t degree = 0;       // 0 = the table's width
    uint32_t expand = 4;
    uint32_t max_iters = 64;
};

struct AnnStats {   // AnnSearchStats (hnsw.rs:266-297) summed over a call; field for field fsgpu_ann_stats
    uint64_t index_size = 0;
    uint32_t dimension = 0, ef_search = 0, k_requested = 0, launches = 0;
    uint64_t queries = 0, approximate = 0, underfilled = 0, empty_despite_indexed_points = 0, rows_scored = 0, steps = 0;
    double device_ms = 0.0;
};

struct CertifiedEf {   // recall_certificate.rs:143-152
    uint32_t ef_search = 0;
    bool meets_target = false;
    double certified_recall = 0.0;
};

// recall_certificate.rs:50-138 in f64; non-finite entries are ignored
double conformal_recall_lower_bound(const double* recalls, uint64_t n, double alpha);
double mean_recall_lower_bound(const double* recalls, uint64_t n, double delta);
double mean_recall_lower_bound_bernstein(const double* recalls, uint64_t n, double delta);
// certified_min_ef / certified_min_ef_mean (recall_certificate.rs:165-230); false for an empty calibration
bool certified_min_ef(const uint32_t* efs, const double* const* recalls, const uint64_t* lens, uint32_t n, double target, double level,
                      bool mean_bound, CertifiedEf* out);
// recall_at_k_of over rows (hnsw.rs:3101-3112)
double recall_at_k_of_rows(const uint32_t* approx, uint32_t n_approx, const uint32_t* exact, uint32_t n_exact);

class AnnIndex {
  public:
    ~AnnIndex();
    AnnIndex() = default;
    AnnIndex(const AnnIndex&) = delete;
    AnnIndex& operator=(const AnnIndex&) = delete;

    // uploads the table; every limit that does not depend on a call (include/fsgpu.h) is checked here, before anything is allocated
    SearchError init(VectorIndex* index, const uint32_t* graph_rows, uint64_t graph_len, uint32_t graph_width, const AnnConfig& config);
    uint64_t record_count() const { return nrows_; }
    int device() const { return device_; }
    VectorIndex* index() const { return index_; }
    // on_device: queries and the four outputs are device pointers (out_flags may be null either way).  Blocks.  The caller holds the
    // index's mutex.
    SearchError search(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t ef, uint32_t* out_rows, float* out_scores,
                       uint32_t* out_counts, uint32_t* out_flags, bool on_device, AnnStats* stats);
    // certify_ef_search: sweep holds n_efs entries
    SearchError certify_ef(const float* queries, uint32_t nq, const uint32_t* candidate_efs, uint32_t n_efs, uint32_t k, double target,
                           double alpha, CertifiedEf* chosen, CertifiedEf* sweep, uint32_t* n_swept);
    const AnnStats& last_stats() const { return last_; }

  private:
    SearchError check_call(uint32_t k, uint32_t ef) const;
    VectorIndex* index_ = nullptr;
    int device_ = -1;   // the index's device, kept here: the destructor frees device memory and must not need the index for it
    uint64_t nrows_ = 0, generation_ = 0;
    uint32_t width_ = 0;
    AnnConfig cfg_;   // as resolved at init: n_entry clamped, degree filled in
    DeviceBuffer graph_, ws_;
    void* pin_ = nullptr;   // pinned block the counts, counters and hits of a call come up through
    size_t pin_bytes_ = 0;
    hipEvent_t ev_begin_ = nullptr, ev_end_ = nullptr;
    AnnStats last_;
};

}  // namespace fsgpu

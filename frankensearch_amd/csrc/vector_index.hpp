// vector_index.hpp — host-side mirror of the reference's VectorIndex / Model2VecEmbedder for the
// device-resident path (names and error behaviour follow crates/frankensearch-index/src/lib.rs:819,
// src/search.rs:192-494 and crates/frankensearch-embed/src/model2vec_embedder.rs:55-58).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "kernels.hpp"

namespace fsgpu {

// SearchError (crates/frankensearch-core/src/error.rs:57-176) carried as code + detail.
struct SearchError {
    int32_t code = 0;
    std::string detail;
    bool ok() const { return code == 0; }
};

struct DeviceBuffer {
    void* ptr = nullptr;
    size_t bytes = 0;
    SearchError reserve(size_t want);
    void release();
};

// VectorIndexWriter for FSVI v1 (lib.rs:3637-3672, 3752-3943): validate, stable-sort by (FNV-1a(doc_id), doc_id), write.
SearchError write_fsvi_v1(const char* path, const char* embedder_id, const char* embedder_revision, uint32_t dim, uint64_t n,
                          const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors,
                          uint8_t compaction_gen, int device, uint8_t quantization = 1);

// ---- a filter per query (vector_index_filtered.cpp) --------------------------------------------------------------------
// What the index needs of a resident filter (fsgpu_allow_bitmap): its words on the device, its popcount and the ascending row list
// the device built from the words (build_filter_row_list, cached on the handle).
struct ResidentFilterView {
    const uint64_t* words_host = nullptr;
    const uint64_t* words_dev = nullptr;
    uint64_t allowed = 0;
    const uint32_t* rows_dev = nullptr;   // [allowed] local row ids, ascending; may be null while allowed * 50 >= record count
};
// The row list of a bitmap over nrows rows with `allowed` set bits, built on `device` (filter_gather_kernels.hip) into *rows; blocks.
SearchError build_filter_row_list(int device, const uint64_t* words_dev, uint64_t nrows, uint64_t allowed, DeviceBuffer* rows);
// Grouping and path decision of a call, host code only.  Groups are numbered in the order their first query appears; a group's
// queries keep ascending query order; filter -1 (no filter) is a group like any other; a filter no query names forms no group.
//   path: unfiltered | dense (allowed * 50 >= nrows: masked batched scan) | gather (0 < allowed * 50 < nrows) | empty (allowed == 0)
enum MultiFilterPath : int32_t { kMultiUnfiltered = 0, kMultiDense = 1, kMultiGather = 2, kMultiEmpty = 3 };
SearchError multi_filter_plan(uint64_t nrows, const uint64_t* allowed_per_filter, uint32_t nfilters, const int32_t* filter_of_query,
                              uint32_t nq, int32_t* out_group_of_query, int32_t* out_path_of_group, int32_t* out_filter_of_group,
                              uint32_t* out_ngroups);

class VectorIndex {
  public:
    VectorIndex();
    ~VectorIndex();
    VectorIndex(const VectorIndex&) = delete;
    VectorIndex& operator=(const VectorIndex&) = delete;

    // VectorIndex::open for a raw slab (host copy) / an adopted device slab / an FSVI v1 file.
    // f32_rows: the slab holds raw little-endian f32 rows (Quantization::F32) instead of f16
    SearchError init_host(int device, uint32_t dim, uint64_t nrows, const void* slab, const uint64_t* live,
                          uint64_t row_base, bool f32_rows = false);
    bool f32_rows() const { return f32_; }
    SearchError init_device(int device, uint32_t dim, uint64_t nrows, const void* slab_dev, const uint64_t* live_dev,
                            uint64_t row_base, bool f32_rows = false);
    SearchError open_fsvi(const char* path, int device);
    // What open_fsvi leaves behind, from parts that never were a file (index_builder.cpp): the slab is a device allocation that
    // becomes this index's own, the tables are the file's record table in memory (hashes [nrows], offsets [nrows + 1] into blob).
    // On failure nothing was taken.
    SearchError adopt_built(int device, uint32_t dim, uint64_t nrows, DeviceBuffer* slab, bool f32_rows, std::vector<uint64_t>* hashes,
                            std::vector<uint64_t>* offsets, std::string* blob, const std::string& embedder_id,
                            const std::string& embedder_revision, uint8_t compaction_gen);
    // catalog of a row-sharded index: the file's tables stay here (doc ids, tombstones, WAL, hit resolution), the slab is handed
    // back in `image` for the shards; topk_override replaces this object's own scan inside search_hits
    struct FsviImage {
        std::vector<uint8_t> bytes;
        size_t slab_offset = 0;
        uint32_t dim = 0;
        uint64_t nrows = 0;
        bool f32_rows = false;
    };
    SearchError open_fsvi_catalog(const char* path, FsviImage* image);
    std::function<SearchError(const float* query, uint32_t k, uint32_t* rows, float* scores, uint32_t* count)> topk_override;
    const std::vector<uint64_t>& live_host() const { return live_host_; }

    uint64_t record_count() const { return nrows_; }
    uint32_t dimension() const { return dim_; }

    // search_top_k over nq queries (host pointers; synchronous).
    // allow_resident_dev: the device copy of `allow` when the caller keeps one (fsgpu_allow_bitmap: a filter reused across
    // searches is uploaded once, not per call); null = `allow` is uploaded for this call
    SearchError search_top_k(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                             const uint64_t* allow, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                             const uint64_t* allow_resident_dev = nullptr);
    // same with device pointers, enqueued on `stream`.
    SearchError search_top_k_device(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                    const uint64_t* allow_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                                    uint32_t* out_counts_dev, hipStream_t stream);
    // Batched search on the matrix cores (mfma_scan.hip): groups of 64 queries per HBM pass, approximate f16-query
    // scores filtered by a proven margin and re-scored in the reference order, so the outputs equal
    // search_top_k_device bit for bit.  Queries it cannot serve (k > 64, unsupported dim, margin overflow) run on the
    // exact kernels.  Synchronises the stream (the fallback decision is taken on the host).
    SearchError search_top_k_batched_device(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                            const uint64_t* allow_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                                            uint32_t* out_counts_dev, hipStream_t stream, uint32_t* fallbacks,
                                            uint64_t* out_packed_dev = nullptr);
    // ... in two halves: begin enqueues the whole search and returns a ticket (0 / 1; two may be outstanding), end waits for that
    // search alone, reads the verdicts and runs the fallbacks.  Queries and outputs stay the caller's until end.
    SearchError search_top_k_batched_device_begin(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                                  const uint64_t* allow_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                                                  uint32_t* out_counts_dev, hipStream_t stream, uint64_t* out_packed_dev, int32_t* ticket);
    // late_answers (may be null): queries whose hits were written by work enqueued in END — exact fallbacks and queries the int8 filter
    // handed to the f16 filter; a caller that ordered work behind begin's last kernel must order it again behind these
    SearchError search_top_k_batched_device_end(int32_t ticket, uint32_t* fallbacks, uint32_t* late_answers = nullptr);
    SearchError search_top_k_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                     const uint64_t* allow, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                     uint32_t* fallbacks, const uint64_t* allow_resident_dev = nullptr,
                                     bool queries_on_device = false);   // queries: a device pointer (an encoder's device output)
    // Batched row-level search in which query q names filters[filter_of_query[q]], or none (-1): per query the rows, score bits and
    // count of search_top_k with that filter's bitmap.  Queries are grouped by filter; unfiltered and dense groups ride
    // search_top_k_batched_device, the selective groups share ONE launch of the segmented gather scan (filter_gather_kernels.hip),
    // an empty filter costs no launch.  Selective groups of a shape the gather scan does not cover (F32 slab, MRL view, dim % 8,
    // k > 256) are answered per query by search_top_k and counted in *fallbacks, together with the batched groups' own fallbacks.
    // Device pointers (queries, outputs) on `stream`, which is synchronised; filter_of_query is a host array.  The filters were
    // checked against this index by the caller; a selective filter's rows_dev must be set.
    SearchError search_top_k_multi_filtered(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                            const ResidentFilterView* filters, uint32_t nfilters, const int32_t* filter_of_query,
                                            uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev, hipStream_t stream,
                                            uint32_t* fallbacks);
    // ... with host pointers (synchronous)
    SearchError search_top_k_multi_filtered_host(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                 const ResidentFilterView* filters, uint32_t nfilters, const int32_t* filter_of_query,
                                                 uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* fallbacks);
    // queries of search_top_k_multi_filtered by path: gather scan, dense-group pass, unfiltered, per-query fallback
    uint64_t multi_gathered = 0, multi_scanned = 0, multi_unfiltered = 0, multi_fallbacks = 0;
    // Batched search_top_k_int8_two_pass (search.rs:514-661): int8 pass 1 on the matrix cores (exact integer scores, so the
    // k*multiplier candidates are exactly the reference's), exact f16 rescore, top-k.  No doc-id dedup (raw row ids).
    SearchError search_top_k_int8_batched_device(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                                 uint32_t multiplier, uint32_t* out_rows_dev, float* out_scores_dev,
                                                 uint32_t* out_counts_dev, hipStream_t stream, uint32_t* fallbacks, int bits = 8);
    // bits = 4: batched search_top_k_4bit_two_pass (search.rs:876-946)
    SearchError search_top_k_int8_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                          uint32_t multiplier, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                          uint32_t* fallbacks, int bits = 8, bool queries_on_device = false);
    // Shard-local HALF of a two-pass search (bits 8: search_top_k_int8_two_pass, 4: search_top_k_4bit_two_pass) for a row-sharded
    // index: this shard's cc = max(k * multiplier, k) pass-1 candidates per query as two aligned packed lists [nq, cc] — position
    // i is one row: its pass-1 entry (integer score as f32 bits | global row) and its exact entry; kEmpty beyond the candidates.
    // The root repeats the selection over all shards' candidates (launch_two_pass_merge).  In two halves (the tickets of
    // search_top_k_batched_device_begin / _end): nothing is waited for in begin.
    SearchError two_pass_candidates_device_begin(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                                 uint32_t multiplier, int bits, uint64_t* approx_out_dev, uint64_t* exact_out_dev,
                                                 hipStream_t stream, int32_t* ticket);
    SearchError two_pass_candidates_device_end(int32_t ticket, uint32_t* fallbacks, uint32_t* late_answers = nullptr);
    // Shard-local search whose result stays packed (score bits << 32 | global row; ~0 padding) for the
    // cross-GPU exchange: out_packed_dev is [nq, k].  Fused tiers only (k <= 256, dim % 8 == 0).
    SearchError search_top_k_packed_device(const float* queries_dev, uint32_t nq, uint32_t query_len, uint32_t k,
                                           const uint64_t* allow_dev, uint64_t* out_packed_dev, hipStream_t stream);
    SearchError gather_dot(const float* query, uint32_t query_len, const uint32_t* rows, uint32_t n, float* out);
    // ... for MANY queries in one launch: out[i] = dot(queries[qidx[i]], row rows[i]) (host arrays; quality_scores_for_hits of a chunk)
    SearchError gather_dot_batched(const float* queries, uint32_t nq, uint32_t query_len, const uint32_t* rows, const uint32_t* qidx, uint32_t n,
                                   float* out);

    // A lone query in two halves (one at a time per index, on the index's own stream): begin enqueues and returns, end waits and
    // writes the hits — search_top_k(query, 1, ...) without a filter is exactly begin + end.  A row-sharded handle begins the query
    // on every shard before it ends any, so the shards' passes run side by side from ONE host thread.
    SearchError lone_exact_begin(const float* query, uint32_t k);
    SearchError lone_exact_end(uint32_t* out_rows, float* out_scores, uint32_t* out_count);   // [k], [k], [1]
    // ... of a two-pass search (bits 8: search_top_k_int8_two_pass, 4: search_top_k_4bit_two_pass), this shard's half: end yields
    // max(k * multiplier, k) candidate pairs (pass-1 entry | exact entry, aligned; kEmpty beyond the candidates)
    SearchError lone_two_pass_begin(const float* query, uint32_t k, uint32_t multiplier, int bits);
    SearchError lone_two_pass_end(uint64_t* out_approx, uint64_t* out_exact);

    // search_top_k + scan_wal + resolve_hits (search.rs:426-494, 1449-1475, 1493-1558): GPU top-k of the main
    // rows, host merge of the resident WAL entries, WAL shadowing and doc-id dedup.  Needs a doc-id table.
    SearchError search_hits(const float* query, uint32_t query_len, uint32_t k, uint32_t* out_rows, float* out_scores,
                            uint32_t* out_count);
    // search_hits for nq queries (vector_index_hits.cpp, search_hits_kernels.hip): the batched search's main rows stay on the device,
    // wal_topk_kernel scores a device mirror of the WAL, resolve_hits_kernel merges, shadows and dedups by doc-id class.  Same rows,
    // score bits and counts as search_hits per query.  *fallbacks: queries answered per query (k = 0, k > 256, >= 2^32 rows + WAL
    // entries) or whose main rows the batched search took from the exact kernels.
    SearchError search_hits_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t* out_rows,
                                    float* out_scores, uint32_t* out_counts, uint32_t* fallbacks, bool queries_on_device = false);
    // search_top_k_{int8,4bit}_two_pass for nq queries on an index with a doc-id table: search_hits_batched when the per-query call
    // takes the exact search (resident WAL, F32 slab, k = 0, no rows), else the row-level batched two-pass + the dedup on the device
    SearchError search_hits_two_pass_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t multiplier,
                                             int bits, uint32_t* out_rows, float* out_scores, uint32_t* out_counts, uint32_t* fallbacks);
    // lab: wal_topk_kernel's score of every resident WAL entry, out [nq, wal_record_count()]
    SearchError lab_wal_scores(const float* queries, uint32_t nq, float* out);
    // VectorIndex::search_top_k_int8_two_pass (search.rs:514-661): int8 pass-1 over the lazily built int8 slab,
    // exact f16 rescore of the k*multiplier candidates; falls back to the exact search when a WAL is resident.
    SearchError search_top_k_int8_two_pass(const float* query, uint32_t query_len, uint32_t k, uint32_t multiplier,
                                           uint32_t* out_rows, float* out_scores, uint32_t* out_count);
    // VectorIndex::search_top_k_4bit_two_pass (search.rs:876-946): packed signed-nibble pass-1 (a quarter of the f16
    // bytes), exact f16 rescore; same fallbacks.
    SearchError search_top_k_4bit_two_pass(const float* query, uint32_t query_len, uint32_t k, uint32_t multiplier,
                                           uint32_t* out_rows, float* out_scores, uint32_t* out_count);
    // VectorIndex::mrl_search_with_stats (crates/frankensearch-index/src/mrl.rs:241-395): truncated scan over the first
    // search_dims dimensions (a strided view of the same slab), resident WAL entries, rescore over rescore_dims, top-k.
    struct MrlStats {
        uint32_t scan_dims = 0, rescore_dims = 0, candidates_rescored = 0;
        uint64_t records_scanned = 0;
        bool fell_back_to_full = false;
    };
    SearchError mrl_search(const float* query, uint32_t query_len, uint32_t k, uint32_t search_dims, uint32_t rescore_dims,
                           uint32_t rescore_top_k, uint32_t* out_rows, float* out_scores, uint32_t* out_count,
                           MrlStats* stats);
    // mrl_search for nq host queries at once: batched truncated scan on the matrix cores + one re-score launch (no stats)
    SearchError mrl_search_batched(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t search_dims,
                                   uint32_t rescore_dims, uint32_t rescore_top_k, uint32_t* out_rows, float* out_scores,
                                   uint32_t* out_counts, uint32_t* fallbacks);
    // VectorIndex::append (lib.rs:2532-2720): resident WAL entry, immediately searchable.
    SearchError wal_append(const char* doc_id, uint32_t len, const float* vector, uint32_t vector_len);
    uint64_t wal_record_count() const { return wal_.size(); }
    SearchError doc_id_at(uint32_t row, const char** ptr, uint32_t* len) const;
    SearchError soft_delete(const char* doc_id, uint32_t len, int32_t* deleted);
    SearchError allow_bitmap_for_hashes(const uint64_t* hashes, uint32_t n, uint64_t* bitmap_out, uint64_t* matched) const;
    SearchError set_live_bitmap(const uint64_t* live);
    bool has_doc_ids() const { return !doc_offsets_.empty(); }
    // record-table accessors for the two-tier alignment (two_tier.rs:758-840) and quality_scores_for_hits (:1566-1631)
    bool row_tombstoned(uint64_t r) const { return !live_host_.empty() && !((live_host_[r >> 6] >> (r & 63)) & 1ull); }
    uint64_t doc_hash_at(uint64_t r) const { return doc_hashes_[r]; }
    // VectorIndex::find_index_by_doc_id (lib.rs:3395-3421): first LIVE main row with this doc id, -1 if none
    int64_t find_index_by_doc_id(const char* doc_id, uint32_t len) const;
    // latest resident WAL entry of a doc id (-1 if none) and its dot_product_f32_f32 with a query
    int64_t wal_latest(const char* doc_id, uint32_t len) const;
    float wal_dot(size_t wal_index, const float* query) const;
    const std::string& wal_doc_id(size_t wal_index) const { return wal_[wal_index].doc_id; }
    const std::vector<float>& wal_vector(size_t wal_index) const { return wal_[wal_index].embedding; }

    // VectorIndex::vector_at_f32 (lib.rs:3142): one row of the slab widened to f32 (out holds dimension() values)
    SearchError vector_at_f32(uint32_t row, float* out);
    // mmr_rerank (crates/frankensearch-fusion/src/mmr.rs:103-319) over rows of this slab, ONE launch for nq pools (mmr_kernels.hip):
    // pool q owns rows / scores / ovr_index / out_order [offsets[q], offsets[q + 1]).  ovr_index (nullable): >= 0 = the candidate's
    // vector is ovr_vectors[index * dim ..] (a WAL entry), its row is not read.  out_sims (nullable, nq == 1): the pool x pool
    // matrix.  Pools beyond mmr_device_pool run the host restatement on vectors fetched from the slab (same bits).
    SearchError mmr_rerank_rows(const uint32_t* rows, const double* scores, const uint32_t* offsets, uint32_t nq, uint32_t k, double lambda,
                                uint32_t candidate_pool, const int32_t* ovr_index, const float* ovr_vectors, uint32_t n_ovr,
                                uint32_t* out_order, uint32_t* out_counts, double* out_sims);
    // the searcher's stage over this index alone (searcher.rs:2696-2745; fsgpu_index_mmr_rerank_docs)
    SearchError mmr_rerank_docs(const char* const* doc_ids, const uint32_t* doc_id_lens, const float* scores, uint32_t n, bool enabled,
                                double lambda, uint32_t candidate_pool, uint32_t* out_order, uint8_t* out_applied);

    // compute_query_hubness (crates/frankensearch-fusion/src/hubness.rs:109-138) over every row of this slab, tombstoned rows too:
    // out[record_count()] = the mean of the row's min(kq, nq) greatest dot_product_f32_f32 similarities to the sample, in the
    // canonical order (include/fsgpu.h).  hubness_kernels.hip for k <= 64 and dim <= 1,024, launched over ranges of kHubLaunchRows
    // rows; else the host restatement over rows fetched in blocks (same bits).  out_topk (nullable): [record_count(), k] selected
    // sims, greatest first.  Host pointers; blocks; own workspaces on the index's stream.
    SearchError compute_query_hubness(const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq, float* out, float* out_topk);
    // The exact k-NN graph over the main slab (include/fsgpu.h, fsgpu_index_build_knn_graph; vector_index_knn.cpp): for the sources
    // first_row .. first_row + n_rows the first m live rows j != i of the row-level search for "row i widened to f32".  The live
    // sources are staged in chunks of kKnnChunk (knn_graph_kernels.hip) and answered by search_top_k_batched_device_begin / _end, two
    // steps in flight; rows, queries and hits stay in HBM.  out_rows [n_rows, m] (kKnnPadRow padding), out_sims nullable.  Host
    // pointers; blocks; takes both tickets.
    SearchError build_knn_graph(uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t* out_rows, float* out_sims);
    struct KnnBuildStats {   // of the last build_knn_graph: what the ridden search reported, summed over the steps
        uint64_t steps = 0, sources = 0, fallbacks = 0, late_answers = 0;
    };
    KnnBuildStats last_knn_build;
    // The graph optimisation over a neighbour table of this index (include/fsgpu.h, fsgpu_knn_graph_optimize; DESIGN 3.20;
    // vector_index_knn_optimize.cpp, knn_optimize_kernels.hip): graph_rows [record_count, width] -> out_rows [record_count, degree],
    // a pure function of the table and row_base.  Host pointers; blocks; its workspace comes and goes with the call; refused while a
    // begun search is outstanding.  The caller has checked the shape (1 <= degree <= width <= kKnnOptMaxWidth).
    struct KnnOptimizeStats {
        uint64_t rows = 0, forward_edges = 0, reverse_edges = 0, zero_in_degree_before = 0, zero_in_degree_after = 0;
        uint32_t max_detour_count = 0;
        double device_ms = 0.0;
    };
    SearchError optimize_knn_graph(const uint32_t* graph_rows, uint32_t width, uint32_t degree, uint32_t* out_rows, KnnOptimizeStats* stats);
    // ... a row shard's half of the sharded build: n live local rows (src_local) widened to f32 into a host block [n, dim]
    SearchError knn_stage_rows_host(const uint32_t* src_local, uint32_t n, float* out);
    // The build's step loop over a source LIST (vector_index_knn.cpp): next_chunk appends up to cap ascending live local rows and says
    // whether more may follow; every drained step's [n, m] lists (global ids, kKnnPadRow / 0.0f padding) reach the sink in the step's
    // pinned block (lists_to_host) or in its device block on `stream`.  The caller has checked m and holds no ticket.
    struct KnnStepLists {
        const uint32_t* src;          // [n] local source rows (host)
        uint32_t n;
        const uint32_t* rows_host;    // lists_to_host: [n, m]
        const float* sims_host;       // ... and [n, m] when sims were asked for
        const uint32_t* src_dev;      // [n] GLOBAL source rows (device)
        const uint32_t* rows_dev;     // [n, m] (device)
        const float* sims_dev;        // [n, m] or null (device)
        hipStream_t stream;           // work on the device lists is enqueued here
    };
    using KnnNextChunk = std::function<bool(std::vector<uint32_t>&, uint32_t)>;
    using KnnStepSink = std::function<SearchError(const KnnStepLists&)>;
    SearchError knn_search_steps(uint32_t cap, uint32_t m, bool want_sims, bool lists_to_host, const KnnNextChunk& next_chunk,
                                 const KnnStepSink& sink);
    // Carrying a k-NN table across a compaction, a vacuum or deletes (include/fsgpu.h, fsgpu_index_update_knn_graph; DESIGN 3.21;
    // vector_index_knn_update.cpp, knn_update_kernels.hip): the table build_knn_graph(0, record_count, m) would return now, from the
    // table of the index as it was and the map new row -> old row.  Rows are classified on the device; added and kept-dirty rows are
    // searched through knn_search_steps; kept-clean lists are the remapped old lists joined against the added rows.  Host pointers;
    // blocks; takes both tickets; its workspace comes and goes with the call.  The caller has checked m, the pointers and the map.
    struct KnnUpdateStats {
        uint64_t rows = 0, dead = 0, added = 0, kept_clean = 0, kept_dirty = 0, searched_sources = 0, join_pairs = 0, join_entries = 0;
        uint32_t rebuilt = 0;
        double device_ms = 0.0, join_ms = 0.0;
    };
    SearchError update_knn_graph(uint32_t m, const uint32_t* old_rows, const float* old_sims, uint64_t old_len, uint32_t old_row_base,
                                 const uint32_t* new_to_old, float max_added_fraction, uint32_t* out_rows, float* out_sims,
                                 KnnUpdateStats* stats);
    // what fsgpu_index_update_knn_graph refuses before any work: the map's entries (pad or < old_len, no predecessor named twice)
    SearchError knn_update_check_map(const uint32_t* new_to_old, uint64_t old_len) const;
    // The last rewrite's map new row -> old main row (kKnnPadRow: from the WAL), kept as runs and expanded here; out [record_count]
    SearchError rewrite_sources(uint32_t* out_new_to_old, uint64_t* generation_before, uint64_t* generation_after, uint64_t* old_record_count) const;
    // The beam search over a k-NN table of this index (ann_index.cpp, ann_kernels.hip): `a` arrives with the table, the parameters,
    // the queries and the outputs; the slab, the live bitmap AS IT IS NOW, the shape and the hreduce order are filled in here.
    // Refused before the launch when the caps of ann_args_ok do not hold.  Enqueues on `stream`.
    SearchError ann_launch(AnnSearchArgs a, uint32_t nq, hipStream_t stream);
    // What the IVF handle (ivf_index.cpp) reads of this index for its own launches: the slab, the live bitmap AS IT IS NOW and the
    // shape.  Refused for an F32 slab, a truncated view, a catalog without a slab.
    struct IvfSlabView {
        const void* slab = nullptr;
        const u64* live = nullptr;   // device; nullptr = all live
        uint32_t nrows = 0, dim = 0, row_base = 0, row_stride = 0;
        int num_cus = 0;
    };
    SearchError ivf_view(IvfSlabView* out) const;
    // The int8 filter's copy as the batched search uses it (built now if need be; no room for it is an error), for a handle that
    // makes a copy of its own: the pointers are good until the index rebuilds or drops its copy.
    struct FilterCopyView {
        const signed char* slab_i8 = nullptr;       // [nrows, dim]
        const unsigned int* max_bits = nullptr;     // the scale word
        const unsigned int* stats = nullptr;        // four words
        bool rotated = false;
        const double* rot_mat = nullptr;            // [dim, dim] when rotated
        double extra_coeff = 0.0;
    };
    SearchError ivf_filter_copy(FilterCopyView* out);

    // VectorIndex::append_batch (lib.rs:2546-2720): every entry validated before anything changes, last-wins dedup inside the batch,
    // resident copies superseded, the first live main row of each doc id tombstoned, ONE live-bitmap upload.  wal_append is a batch of one.
    SearchError wal_append_batch(uint32_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors, uint32_t vector_len);
    // VectorIndex::compact / vacuum / rewrite_index (lib.rs:2734-2854, 2485-2521, 2871-3094) on the device-resident slab
    // (vector_index_compact.cpp, compact_kernels.hip): the host merges the sorted record table with the sorted WAL into RUNS of
    // surviving rows, the device copies them into a fresh slab, the tables are rebuilt, everything derived from row ids or slab bytes is
    // dropped.  path (nullable): the new FSVI image is also written beside it and renamed over it.  On failure nothing has changed.
    struct CompactionStats {
        uint64_t main_records_before = 0, wal_records = 0, total_records_after = 0;
        double elapsed_ms = 0.0;
    };
    struct VacuumStats {
        uint64_t records_before = 0, records_after = 0, tombstones_removed = 0, bytes_reclaimed = 0;
        double elapsed_ms = 0.0;
    };
    SearchError compact(const char* path, CompactionStats* out);
    SearchError vacuum(const char* path, VacuumStats* out);
    // needs_compaction (lib.rs:2270-2292) with WalConfig's two numbers as arguments; needs_vacuum (lib.rs:174, 2464-2475)
    bool needs_compaction(uint64_t threshold, double ratio) const;
    bool needs_vacuum() const { return nrows_ != 0 && (double)tombstone_count() / (double)nrows_ > 0.20; }   // strict
    // (an adopted device slab came with a device bitmap only: fetch_live_host brings it down once, before anything counts tombstones)
    SearchError fetch_live_host();
    uint64_t tombstone_count() const;
    uint64_t live_count() const { return nrows_ - tombstone_count(); }
    uint64_t generation() const { return generation_; }   // rewrites that changed the slab since the handle was made
    uint8_t compaction_gen() const { return compaction_gen_; }
    // lab: rows one launch of the compaction kernel covers (0 = kCompactLaunchRows) and its stores' cache policy; what the last rewrite cost
    uint32_t compact_launch_rows = 0;
    bool compact_nt_stores = false;
    struct RewriteTimes {
        double plan_ms = 0, kernel_ms = 0, tables_ms = 0, file_ms = 0, rebuild_ms = 0;
        uint64_t runs = 0, launches = 0, dst_bytes = 0;
    };
    RewriteTimes last_rewrite;
    // lab: a doc-id table for an index made from a bare slab ("doc-000000000" ... in (hash, doc id) order over the rows as they are),
    // so that the write path can be measured on a generated corpus that never was a file
    SearchError lab_attach_synthetic_doc_ids();

    std::mutex& mutex() { return mu_; }
    int device() const { return device_; }
    int32_t hreduce = 0;
    int32_t variant = 0;
    uint64_t filter_gathered = 0, filter_scanned = 0;  // filtered host searches by path
    bool profiling = false;
    int profile_period = 1;   // fsgpu_index_set_profiling(n > 1): the merged main launch of every n-th batched step is timed
    uint32_t profile_tick_ = 0;
    // one-shot hook of the next batched search (fsgpu_index_set_after_enqueue_hook): called before the search blocks on its stream
    void (*after_enqueue_fn)(void*) = nullptr;
    void* after_enqueue_ctx = nullptr;
    // filter of the exact batched search (fsgpu_index_set_batched_filter): 0 = automatic, 1 = f16 slab, 2 = int8 slab
    int32_t batched_filter = 0;
    // fsgpu_index_set_int8_latency: unfiltered fsgpu_search_topk calls of a few queries go through the int8 filter too
    bool int8_latency = false;
    bool int8_latency_build_now = false;   // FSGPU_INT8_LATENCY_BUILD_NOW is in force: a rewrite of the slab rebuilds the copies before it returns
    // fsgpu_index_set_filter_rotation: 0 = automatic (rotate the filter's copy when the slab has outlier channels), 1 = never, 2 = always.
    // Takes effect when the filter's copy is built (first batched search / fsgpu_index_int8_filter_bound).
    int32_t filter_rotation = 0;
    bool filter_rotated() const { return i8f_rot_; }
    bool exact_only_ = false;   // fsgpu_search_topk_exact: the call in flight takes the exact kernels whatever copies the index holds
    // Which bits of (score sortkey << 32 | ~row) can differ over this slab's rows: all of the score half, the row bits below the
    // highest one in which the first and the last row id differ — unless empty entries (key 0: tombstoned / filtered rows) are among them.
    uint64_t sortkey_varying_bits(bool may_hold_empty) const {
        if (may_hold_empty || nrows_ == 0) return ~0ull;
        const uint64_t lo = row_base_, hi = row_base_ + nrows_ - 1;
        uint64_t x = (lo ^ hi) & 0xffffffffull, mask = 0;
        while (x) {
            mask = (mask << 1) | 1ull;
            x >>= 1;
        }
        return 0xffffffff00000000ull | mask;
    }
    SearchError prepare_int8_latency();   // builds the int8 copy + its statistics now (else: the first batched search does)
    uint64_t i8f_queries = 0, i8f_refiltered = 0;  // queries the int8 filter took / handed on to the f16 filter
    bool int8_filter_active() const { return batched_filter == 2 || (batched_filter == 0 && !i8f_disabled_); }
    // The certificate of the int8 filter, for inspection: per query the bound delta on |int8 score - exact score x slab scale
    // x query scale| (< 0: not certifiable) and the query scale 127 / max|q|; the slab scale 127 / max|x|; the quantised queries
    // (nq x dim int8) and, when out_slab_i8 is given, the int8 slab (nrows x dim).  Builds the int8 slab if need be.
    SearchError int8_filter_bound(const float* queries, uint32_t nq, uint32_t query_len, float* out_delta, float* out_query_scale,
                                  float* out_slab_scale, int8_t* out_queries_i8, int8_t* out_slab_i8);
    // a row shard of a larger index: its max-abs for the cross-shard reduction, then the corpus-wide value adopted as THE scale
    SearchError compute_local_quant_max(unsigned int** max_bits_dev, hipStream_t stream);
    void adopt_global_quant_max();
    hipStream_t stream() const { return stream_; }
    VectorIndex* mrl_view(uint32_t dims);  // strided prefix view of this slab (created on first use)
    // Concurrent callers (the reference's scan is `&self`, lock-free, any number of callers: search.rs:192): replicas of this
    // index over the SAME slab and live bitmap, each with its own stream, workspaces and mutex, so that row-level searches from
    // different host threads run side by side instead of queueing on one stream.  The caller holds the owner's state lock.
    static constexpr size_t kLanes = 4;                // this index + 3 replicas
    SearchError ensure_replicas();                      // idempotent
    VectorIndex* replica(size_t i) { return i < replicas_.size() ? replicas_[i].get() : nullptr; }
    size_t replica_count() const { return replicas_.size(); }
    void sync_replicas();                               // after a mutation: live bitmap pointer, hreduce, variant
    SearchError scan_time(double* total_ms, uint64_t* launches, uint64_t* rows, bool reset);

  private:
    SearchError ensure_query_dimension(uint32_t query_len) const;
    SearchError open_fsvi_impl(const char* path, int device, FsviImage* image);
    void* pinned_io();
    // The batched search (vector_index_batched.cpp): its request, outcome, plan, round and ticket are defined in vector_index_internal.hpp
    struct BatchedRequest;
    struct BatchedOutcome;
    struct BatchedPlan;
    struct BatchedRound;
    struct BatchedTicket;
    SearchError batched_impl(const BatchedRequest& rq, BatchedOutcome* out);
    SearchError batched_exact(BatchedRequest& rq, BatchedOutcome* out);   // picks the filter of the exact search, keeps its accounts
    SearchError batched_prepare(BatchedPlan& p, bool* usable);
    SearchError batched_unusable(const BatchedPlan& p, BatchedOutcome* out);
    SearchError batched_round_setup(const BatchedPlan& p, BatchedRound& r, uint32_t g0);
    SearchError batched_sample(const BatchedPlan& p, BatchedRound& r);
    SearchError batched_main(const BatchedPlan& p, BatchedRound& r);
    SearchError batched_finish(const BatchedPlan& p, BatchedRound& r);
    SearchError batched_fallback(const BatchedPlan& p, BatchedOutcome* out, bool already_waited = false);
    void i8f_account(uint32_t nq, uint32_t refiltered);
    SearchError quantized_two_pass(const float* query, uint32_t query_len, uint32_t k, uint32_t multiplier, int bits,
                                   uint32_t* out_rows, float* out_scores, uint32_t* out_count, u64* approx_out_dev = nullptr,
                                   u64* exact_out_dev = nullptr);
    // The lone query of the int8 latency path: ONE fused pass over the int8 slab that keeps the 256 best integer scores
    // (scan_i8_topk_kernel, 0.75 of HBM peak), their exact re-score, and a certificate — the 256th integer score lies more than
    // 2 delta below the k-th, so every row that could reach the exact top k was among them.  *certified = false: nothing was
    // written, the staged filter path answers.
    SearchError certified_i8_lone_query(const float* query, uint32_t k, uint32_t* out_rows, float* out_scores, uint32_t* out_count,
                                        bool* certified);
    SearchError two_pass_lone_certified(const float* query, const unsigned char* qi, uint32_t qbytes, uint32_t k, uint32_t k_eff, uint32_t cc,
                                        int bits, const void* qslab, uint32_t* rows, float* scores, uint32_t* count, bool* answered);
    // ... and the halves of both lanes (enqueue only / one synchronisation + the certificate)
    SearchError certified_i8_enqueue(const float* query, uint32_t k, bool* enqueued);
    SearchError certified_i8_check(uint32_t* out_rows, float* out_scores, uint32_t* out_count, bool* certified);
    SearchError two_pass_lone_enqueue(const float* query, const unsigned char* qi, uint32_t qbytes, uint32_t k, uint32_t k_eff, uint32_t cc,
                                      int bits, const void* qslab, bool want_pairs, bool* enqueued);
    SearchError two_pass_lone_check(uint32_t* rows, float* scores, uint32_t* count, u64* approx_out, u64* exact_out, bool* answered);
    SearchError ensure_two_pass_slab(int bits, const void** qslab);
    // the int8 filter's copy of the slab, its scale word and statistics: the reference's own int8 slab (shared with the two-pass
    // search), or a ROTATED copy of its own (vector_index_batched.cpp, "the int8 filter's copy of the slab")
    static constexpr double kRotateRatio = 9.0;   // max |element| x sqrt(dim) / max row norm above which the copy is rotated
    // (an F32 slab's copy is always one of its own, rotated or not: i8_slab_ is the reference's int8 slab of an F16 index, which the
    // two-pass searches read and an F32 index does not have)
    bool filter_own() const { return i8f_rot_ || f32_; }
    bool filter_ready() const { return filter_own() ? i8f_ready_ : (i8_ready_ && i8_stats_ready_); }
    const void* filter_slab() const { return filter_own() ? i8f_slab_.ptr : i8_slab_.ptr; }
    const unsigned int* filter_max() const { return static_cast<const unsigned int*>(filter_own() ? i8f_max_.ptr : i8_max_.ptr); }
    const unsigned int* filter_stats() const { return static_cast<const unsigned int*>(filter_own() ? i8f_stats_.ptr : i8_stats_.ptr); }
    bool dense_rows() const { return !row_stride_ || row_stride_ == dim_ * (f32_ ? 4u : 2u); }   // not an MRL prefix view
    SearchError ensure_filter_copy(hipStream_t stream, bool must = false);   // decides the rotation on first use; builds what is missing
    SearchError prepare_filter_queries(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t q_stride, void* qi8, float* delta, float* unit,
                                       hipStream_t stream);
    DeviceBuffer i8f_slab_, i8f_max_, i8f_stats_, rot_mat_, rot_q_;
    bool i8f_decided_ = false, i8f_rot_ = false, i8f_ready_ = false;
    double rot_extra_coeff_ = 0.0;
    enum LoneKind : int {
        kLoneNone = 0, kLoneEmpty, kLoneUnpinned, kLoneCertified, kLoneStaged, kLoneStagedBlocking, kLoneExact,
        kLoneTwoPassLane, kLoneTwoPassBatched, kLoneTwoPassBlocking
    };
    struct LoneState {   // the lone query in flight (lone_*_begin .. lone_*_end)
        int kind = kLoneNone;
        const float* query = nullptr;   // the caller's, valid until end
        uint32_t k = 0, mult = 0, cc = 0, cc_out = 0;
        int bits = 8;
        int32_t ticket = -1;
        bool staged_behind = false;     // a failed certificate is followed by the staged filter path (opt-in) / the exact kernels (default)
    };
    LoneState lone_;
    uint32_t cert_k_ = 0;   // k of the certified pass in flight
    struct TwoPassLane {    // the two-pass lane in flight: its k, candidate count and offsets into the pinned staging block
        uint32_t k = 0, cc = 0;
        size_t o_out = 0, o_flags = 0, o_approx = 0, o_exact = 0;
    };
    TwoPassLane tp_lane_;
    SearchError common_init(int device);
    // rewrite_index: `sources` in output order — a main row, or (kWalSource | WAL index)
    static constexpr uint64_t kWalSource = 1ull << 63;
    SearchError rewrite(const std::vector<uint64_t>& sources, uint8_t new_gen, bool clear_wal, const char* path);
    SearchError rewrite_refusal() const;
    void drop_derived_state();
    uint64_t fsvi_image_bytes(uint64_t rows, uint64_t strings_len) const;
    SearchError fused_search(const float* queries_dev, uint32_t nq, uint32_t k_out, uint32_t k_eff,
                             const uint64_t* allow_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                             uint32_t* out_counts_dev, u64* out_packed_dev, hipStream_t stream);
    hipError_t gather_dot_any(const ScanArgs& a, const uint32_t* rows, uint32_t n, float* out, hipStream_t stream) const;
    SearchError gather_search(const float* queries_dev, uint32_t nq, uint32_t k, const uint32_t* rows_dev, uint32_t n,
                              uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev, hipStream_t stream);
    SearchError general_search(const float* queries_dev, uint32_t nq, uint32_t k_out, uint32_t k_eff,
                               const uint64_t* allow_dev, uint32_t* out_rows_dev, float* out_scores_dev,
                               uint32_t* out_counts_dev, hipStream_t stream);
    ScanArgs base_args(const float* queries_dev, const uint64_t* allow_dev) const;

    std::mutex mu_;
    int device_ = -1;
    int num_cus_ = 256;
    uint32_t dim_ = 0;
    uint64_t nrows_ = 0;
    uint64_t row_base_ = 0;
    uint32_t row_stride_ = 0;  // bytes between rows; dim_*2 except for the MRL prefix views
    std::map<uint32_t, std::unique_ptr<VectorIndex>> views_;  // strided prefix views of this slab, by dimension
    std::vector<std::unique_ptr<VectorIndex>> replicas_;      // lanes for concurrent row-level searches
    const void* slab_dev_ = nullptr;
    const uint64_t* live_dev_ = nullptr;
    bool owns_slab_ = false;
    bool f32_ = false;  // Quantization::F32 slab: the exact kernels of f32_kernels.hip; batches through the int8 filter
    bool catalog_only_ = false;  // the tables of a sharded index: no device state of its own
    DeviceBuffer slab_own_, live_own_;
    hipStream_t stream_ = nullptr;
    // workspaces (grown on demand, reused)
    DeviceBuffer ws_partial_, ws_queries_, ws_allow_, ws_rows_, ws_scores_, ws_counts_, ws_keys_a_, ws_keys_b_,
        ws_sort_tmp_, ws_gather_rows_, ws_gather_out_, i8_slab_, n4_slab_, i8_max_, ws_i8_query_, ws_cand_packed_,
        ws_cand_rows_, ws_cand_scores_, mf_max_norm_, mf_qh_, mf_delta_, mf_tau_, mf_cand_, mf_dense_, mf_sel_,
        mf_fallback_, mf_fallback2_, mf_spill_, mf_io_, mf_io2_, i8_stats_, n4u_slab_, mf_cand_count_, ws_pairs_;
    DeviceBuffer ws_out_;   // rows | scores | counts of a blocking batched search (one block: one copy up)
    // search_top_k_multi_filtered: index | descriptors | grouped queries | grouped hits; the (query, block) lists; the host form's
    // queries and outputs; the host image of the first block's head (alive until the call has synchronised)
    DeviceBuffer ws_multi_, ws_multi_lists_, ws_multi_io_;
    std::vector<unsigned char> multi_host_;
    DeviceBuffer ws_mmr_in_, ws_mmr_out_, ws_mmr_sims_, ws_mmr_vec_;   // mmr_rerank_rows: inputs (one copy down), order | counts, matrix, staged rows
    DeviceBuffer ws_hub_q_, ws_hub_out_, ws_hub_topk_;   // compute_query_hubness: the sample, the table, the selected sims (lab)
    DeviceBuffer ws_knn_[2];   // build_knn_graph: per step in flight  queries | sources | hit rows | hit scores | counts | out rows | out sims
    // search_hits_batched: the doc-id classes of the main rows (dropped with the record table: compact / vacuum); the f32 mirror of
    // the WAL, its entries' classes and the shadowed-row bitmap (dropped by every change of the WAL or the tombstones); one block
    // for a call's  queries | main rows | scores | counts | WAL lists | out rows | scores | counts
    DeviceBuffer hits_main_class_, hits_wal_, hits_wal_class_, hits_shadow_, ws_hits_;
    bool hits_main_ready_ = false, hits_wal_ready_ = false;
    void invalidate_hits_state(bool main_too) {
        hits_wal_ready_ = false;
        if (main_too) hits_main_ready_ = false;
    }
    SearchError ensure_hits_state();
    SearchError hits_per_query(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t* out_rows, float* out_scores,
                               uint32_t* out_counts, uint32_t* fallbacks, bool queries_on_device, uint32_t multiplier, int bits);
    bool i8_ready_ = false, n4_ready_ = false, i8_stats_ready_ = false, n4u_ready_ = false;
    bool quant_max_ready_ = false;   // i8_max_ holds a corpus-wide max-abs handed in by a sharded index: the quantisers keep it
    bool i8f_disabled_ = false;   // the int8 filter left too many queries uncertified on this slab (or its copy does not fit)
    uint32_t i8f_strikes_ = 0;
    uint32_t cert_skip_ = 0, cert_backoff_ = 0;   // the lone query's single-pass certificate: calls still to skip / the current back-off
    uint32_t tp_skip_ = 0, tp_backoff_ = 0;       // ... and the two-pass searches' lone-caller lane
    // search_top_k_batched_device_begin / _end, two_pass_candidates_device_begin / _end: the two tickets
    std::unique_ptr<BatchedTicket[]> tickets_;
    int claim_ticket(uint32_t nq);      // a free ticket, marked finished-in-begin until its search parks; -1: both are out
    bool any_search_parked() const;     // a begun search's kernels may still be reading the slab, the live bitmap and the workspaces
    uint32_t tickets_taken() const;     // parked or finished in begin, not yet ended
    uint32_t i8f_sample_boost_ = 1;   // 1 or 2: the second sample of the int8 filter's wide rounds grows before the filter is given up
    bool mf_norm_ready_ = false;
    int mf_shape_i8_ = 4, mf_per_cu_160_ = 1, mf_per_cu_160_i8_ = 1;
    bool mf_use_160_ = false;
    int mf_per_cu_wide_main_ = 1;  // mfma_wide.hip: one 512-thread block per CU (its LDS ring + candidate lists take ~130 KB)
    int mf_shape_ = -1, mf_per_cu_narrow_ = 1, mf_per_cu_wide_ = 1, mf_per_cu_narrow_i8_ = 1, mf_per_cu_wide_i8_ = 1;  // batched-scan launch shapes (probed once)
    static constexpr size_t kPinnedIoBytes = 256 * 1024;
    void* io_host_ = nullptr;  // pinned staging for the single-query latency paths
    void* batch_io_host_ = nullptr;   // pinned block the results of batched searches come up through (pinned_batch_io)
    size_t batch_io_bytes_ = 0;
    bool batch_io_failed_ = false;
    void* pinned_batch_io(size_t bytes);
    SearchError fetch_batched_results(const unsigned char* base, size_t o_rows, size_t o_scores, size_t o_counts, size_t total, uint32_t nq,
                                      uint32_t k, uint32_t* out_rows, float* out_scores, uint32_t* out_counts);
    const float* host_query_hint_ = nullptr;   // search_top_k's lone query, still in host memory: fused_search launches the scan with it in the argument block
    bool io_failed_ = false;
    uint32_t* mf_flags_host_ = nullptr;                              // pinned per-query verdicts of the batched scan
    uint32_t mf_flags_cap_ = 0;
    // profiling events
    std::vector<std::pair<hipEvent_t, hipEvent_t>> events_;
    uint32_t mf_pass_parity_ = 0;  // main passes of the batched path alternate their direction over the slab
    uint64_t profiled_rows_ = 0;  // slab rows streamed by the timed launches
    uint32_t profiled_elem_bytes_ = 2;
    // FSVI host-side tables
    std::vector<uint64_t> live_host_;
    std::vector<uint64_t> doc_hashes_;
    std::vector<uint64_t> doc_offsets_;  // nrows+1 offsets into doc_blob_
    std::string doc_blob_;
    // resident WAL entries (crates/frankensearch-index/src/wal.rs WalEntry)
    struct WalEntry {
        std::string doc_id;
        std::vector<float> embedding;
    };
    std::vector<WalEntry> wal_;
    // what parse_header keeps of an FSVI file (IndexMetadata, lib.rs:4049-4144): rewrite_index writes it back
    std::string embedder_id_, embedder_revision_;
    uint8_t compaction_gen_ = 0;
    uint16_t publication_nonce_ = 0;
    bool from_fsvi_ = false;
    uint64_t generation_ = 0;
    // the last successful rewrite, as runs of consecutive sources (rewrite_sources expands them): a run starts at new row `first` and
    // copies old main rows from `src` on, or comes from the WAL (src = kWalSource); the last entry is the end marker {record_count, 0}
    struct RewriteRun {
        uint64_t first, src;
    };
    std::vector<RewriteRun> rewrite_runs_;
    uint64_t rewrite_old_rows_ = 0, rewrite_generation_ = 0;   // record_count before it; generation_ after it (0: none happened)
};

class Model2VecEmbedder {
  public:
    ~Model2VecEmbedder();
    SearchError init(int device, const float* table, uint32_t vocab, uint32_t dim);
    // out_dev (on this embedder's device, may be null): the vectors are left in device memory; out (may then be null): host copy
    SearchError embed_batch(const uint32_t* ids, const uint32_t* offsets, uint32_t n, float* out, float* out_dev = nullptr);
    // ... over ids and offsets [n + 1] that already lie in this embedder's device memory, complete (the device tokenizer's CSR)
    SearchError embed_batch_device_ids(const uint32_t* ids_dev, const uint32_t* offsets_dev, uint32_t n, float* out, float* out_dev);
    uint32_t dimension() const { return dim_; }
    int device() const { return device_; }

  private:
    std::mutex mu_;
    int device_ = -1;
    uint32_t vocab_ = 0, dim_ = 0;
    DeviceBuffer table_, ids_, offsets_, out_;
    hipStream_t stream_ = nullptr;
};

SearchError merge_packed_lists_device(int device, const uint64_t* lists_dev, uint32_t nq, uint32_t nlists,
                                      uint32_t list_len, uint64_t q_stride, uint64_t l_stride, uint32_t k,
                                      uint32_t* out_rows_dev, float* out_scores_dev, uint32_t* out_counts_dev,
                                      hipStream_t stream);

}  // namespace fsgpu

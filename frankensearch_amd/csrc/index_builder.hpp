// index_builder.hpp — the device-resident index builder (include/fsgpu.h, "encoder -> index"): VectorIndexWriter's
// write_record + finish (crates/frankensearch-index/src/lib.rs:3607-3672, 3752-3943) for vectors that already sit in device memory.
#pragma once

#include <functional>
#include <mutex>
#include <string>
#include <unordered_set>
#include <vector>

#include "vector_index.hpp"

namespace fsgpu {

class IndexBuilder {
  public:
    struct Options {
        uint8_t quantization = 1;   // Quantization::{F32 = 0, F16 = 1} (lib.rs:203-208)
        uint8_t compaction_gen = 0;
        bool reject_duplicates = false;
        uint32_t chunk_rows = 0;    // 0 = kDefaultChunkRows
        uint64_t reserve_rows = 0;
    };
    struct Stats {
        uint64_t rows = 0, chunks = 0, ingest_launches = 0, permute_launches = 0;
        double ingest_ms = 0, sort_ms = 0, permute_ms = 0, tables_ms = 0, file_ms = 0;
        double ingest_device_ms = 0, permute_device_ms = 0;   // between two events on the stream, around the launches
        uint64_t peak_device_bytes = 0;
    };
    static constexpr uint32_t kDefaultChunkRows = 1u << 16;
    static constexpr uint32_t kHostSliceRows = 1u << 16;   // rows of a host-memory add that are uploaded and ingested at a time

    IndexBuilder() = default;
    ~IndexBuilder();
    IndexBuilder(const IndexBuilder&) = delete;
    IndexBuilder& operator=(const IndexBuilder&) = delete;

    SearchError init(int device, uint32_t dim, const char* embedder_id, const char* embedder_revision, const Options& options);
    // vectors: host memory (on_device = false: the builder's own stream) or memory of the builder's device, ingested behind `stream`
    SearchError add(uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors, uint32_t vector_len,
                    bool on_device, hipStream_t stream, uint64_t* out_bad_row);
    // embed(out_dev) fills the builder-owned [n, dim] device buffer and returns when it is complete
    SearchError add_embedded(const std::function<SearchError(float*)>& embed, int embedder_device, uint32_t embedder_dim, uint32_t n,
                             const char* const* doc_ids, const uint32_t* doc_id_lens, uint64_t* out_bad_row);
    SearchError finish(const char* path, VectorIndex* out, Stats* stats);
    uint64_t record_count() const { return count_; }
    int device() const { return device_; }
    uint32_t dimension() const { return dim_; }

  private:
    SearchError ensure_chunks(uint64_t rows);
    SearchError add_locked(uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors, bool on_device,
                           hipStream_t stream, uint64_t* out_bad_row);
    SearchError write_file(const char* path, const std::vector<uint64_t>& hashes, const std::vector<uint64_t>& offsets,
                           const std::string& blob, const DeviceBuffer& slab) const;
    void release_staging();

    std::mutex mu_;
    int device_ = -1;
    uint32_t dim_ = 0, row_bytes_ = 0, chunk_rows_ = 0;
    Options opt_;
    std::string embedder_id_, embedder_revision_;
    bool spent_ = false;
    uint64_t count_ = 0;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev0_ = nullptr, ev1_ = nullptr;   // around the launches of a call: the device's own time for the stats
    // staging: chunks of chunk_rows_ rows, never moved; the device table of their addresses is rewritten when one is added and holds
    // the first table_rows_ of them (== chunks_.size() between calls: ensure_chunks is all-or-nothing)
    std::vector<void*> chunks_;
    DeviceBuffer table_dev_, verdict_dev_, upload_, embed_out_;
    size_t table_cap_ = 0, table_rows_ = 0;
    unsigned long long* verdict_host_ = nullptr;   // pinned
    // the records in arrival order: FNV-1a of the doc id (computed at add time), the ids back to back
    std::vector<uint64_t> hashes_, id_offsets_{0};
    std::string id_blob_;
    std::unordered_set<std::string> seen_;   // reject_duplicates only
    Stats stats_;
};

}  // namespace fsgpu

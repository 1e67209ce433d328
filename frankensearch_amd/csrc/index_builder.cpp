// index_builder.cpp — host side of the device-resident index builder (include/fsgpu.h, "encoder -> index").
//
// Restated from crates/frankensearch-index/src/lib.rs:
//   write_record_with_flags  :3635-3673   dimension, finite elements, usable norm (vector_signal_usable :6133-6142), doc id <= u16 bytes
//   finish                   :3752-3943   stable sort by (FNV-1a(doc id), doc id) :3753-3762, header | records | strings | pad to 64 | slab
// and from two_tier.rs:2125-2132 (TwoTierIndexBuilder's duplicate rule).  The vector work is two kernels (index_build_kernels.hip):
// every add is validated and encoded into the staging chunks by one pass over its rows, finish gathers the staged rows into the slab
// in file order.  The sort and the tables are host bookkeeping over doc ids, as compaction's merge plan is.  The finished slab is
// handed to a VectorIndex as it stands (VectorIndex::adopt_built): it never visits the host unless a file is asked for.
#include "index_builder.hpp"

#include <unistd.h>

#include <chrono>
#include <cstdio>

#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

namespace {

double ms_since(std::chrono::steady_clock::time_point t0) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

constexpr uint64_t kMaxLaunchElems = (1ull << 31) - 1;   // launch_build_ingest: rows x dim of one launch

}  // namespace

// What open_fsvi_impl + init_host leave behind, without the file: the same fields in the same state.
SearchError VectorIndex::adopt_built(int device, uint32_t dim, uint64_t nrows, DeviceBuffer* slab, bool f32_rows, std::vector<uint64_t>* hashes,
                                     std::vector<uint64_t>* offsets, std::string* blob, const std::string& embedder_id,
                                     const std::string& embedder_revision, uint8_t compaction_gen) {
    if (dim == 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "dimension must be greater than zero");
    if (nrows >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row ids must fit in u32 (VectorHit.index)");
    if (!slab || !slab->ptr) return make_error(FSGPU_ERR_NULL_ARGUMENT, "slab is null");
    if (hashes->size() != nrows || offsets->size() != nrows + 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "record table of another size");
    FSGPU_TRY(common_init(device));
    dim_ = dim;
    nrows_ = nrows;
    row_base_ = 0;
    f32_ = f32_rows;
    // no record carries a flag: every row live, the bitmap present as the reader builds it (lib.rs:1780-1816)
    std::vector<uint64_t> live((size_t)((nrows + 63) / 64), 0);
    for (uint64_t r = 0; r < nrows; ++r) live[(size_t)(r >> 6)] |= 1ull << (r & 63);
    FSGPU_TRY(set_live_bitmap(live.data()));
    slab_own_ = *slab;
    *slab = DeviceBuffer{};
    slab_dev_ = slab_own_.ptr;
    owns_slab_ = true;
    doc_hashes_.swap(*hashes);
    doc_offsets_.swap(*offsets);
    doc_blob_.swap(*blob);
    embedder_id_ = embedder_id;
    embedder_revision_ = embedder_revision;
    compaction_gen_ = compaction_gen;
    publication_nonce_ = 0;
    from_fsvi_ = true;
    return ok();
}

IndexBuilder::~IndexBuilder() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    release_staging();
    for (DeviceBuffer* b : {&verdict_dev_, &upload_, &embed_out_}) b->release();
    if (verdict_host_) (void)hipHostFree(verdict_host_);
    for (hipEvent_t e : {ev0_, ev1_})
        if (e) (void)hipEventDestroy(e);
    if (stream_) (void)hipStreamDestroy(stream_);
}

void IndexBuilder::release_staging() {
    for (void* c : chunks_) (void)hipFree(c);
    chunks_.clear();
    table_dev_.release();
    table_cap_ = 0;
    table_rows_ = 0;
}

SearchError IndexBuilder::init(int device, uint32_t dim, const char* embedder_id, const char* embedder_revision, const Options& options) {
    if (!embedder_id || !embedder_revision) return make_error(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (options.quantization > 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "quantization must be 0 (F32) or 1 (F16)");
    if (dim == 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "dimension must be greater than zero");
    if (dim > (1u << 28)) return make_error(FSGPU_ERR_INVALID_CONFIG, "dimension beyond 2^28");
    const size_t idl = std::strlen(embedder_id), rvl = std::strlen(embedder_revision);
    if (idl > 0xffff || rvl > 0xffff) return make_error(FSGPU_ERR_INVALID_CONFIG, "embedder id / revision must fit in u16");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return make_error(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (device < 0 || device >= count) return make_error(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
    FSGPU_HIP(hipSetDevice(device));
    device_ = device;
    dim_ = dim;
    opt_ = options;
    row_bytes_ = dim * (options.quantization == 1 ? 2u : 4u);
    chunk_rows_ = options.chunk_rows ? options.chunk_rows : kDefaultChunkRows;
    embedder_id_.assign(embedder_id, idl);
    embedder_revision_.assign(embedder_revision, rvl);
    FSGPU_HIP(hipStreamCreateWithFlags(&stream_, hipStreamNonBlocking));
    FSGPU_HIP(hipEventCreate(&ev0_));
    FSGPU_HIP(hipEventCreate(&ev1_));
    FSGPU_TRY(verdict_dev_.reserve(8));
    FSGPU_HIP(hipHostMalloc(reinterpret_cast<void**>(&verdict_host_), 8, hipHostMallocDefault));
    if (options.reserve_rows) FSGPU_TRY(ensure_chunks(options.reserve_rows));
    return ok();
}

// Staging for `rows` rows: whole chunks are added, nothing staged moves.  No kernel of this builder is in flight between calls
// (every add returns with its verdict), so the table of chunk addresses may be replaced.  All or nothing: the decision is taken from
// what the device table holds (table_rows_), a chunk allocated by a call that fails is freed again, and the table in use is
// released only after its successor is allocated and filled, so a refused call leaves chunks_, the table and their agreement as
// they were.
SearchError IndexBuilder::ensure_chunks(uint64_t rows) {
    const size_t need = (size_t)((rows + chunk_rows_ - 1) / chunk_rows_);
    if (need <= table_rows_) return ok();
    const size_t had = chunks_.size();
    auto roll_back = [&]() {
        while (chunks_.size() > had) {
            (void)hipFree(chunks_.back());
            chunks_.pop_back();
        }
    };
    chunks_.reserve(std::max(need, had));
    while (chunks_.size() < need) {
        void* p = nullptr;
        const hipError_t he = hipMalloc(&p, (size_t)chunk_rows_ * row_bytes_);
        if (he != hipSuccess || !p) {
            (void)hipGetLastError();
            roll_back();
            return hip_fail(he != hipSuccess ? he : hipErrorOutOfMemory, "allocation of a staging chunk");
        }
        chunks_.push_back(p);
    }
    DeviceBuffer grown;
    DeviceBuffer* table = &table_dev_;
    size_t cap = table_cap_;
    if (chunks_.size() > table_cap_) {
        cap = table_cap_ ? table_cap_ : 64;
        while (cap < chunks_.size()) cap *= 2;
        const SearchError e = grown.reserve(cap * sizeof(void*));
        if (!e.ok()) {
            roll_back();
            return e;
        }
        table = &grown;
    }
    // (the whole table: in place only entries past table_rows_ change, and no launch has read those)
    const hipError_t he = hipMemcpy(table->ptr, chunks_.data(), chunks_.size() * sizeof(void*), hipMemcpyHostToDevice);
    if (he != hipSuccess) {
        grown.release();
        roll_back();
        return hip_fail(he, "upload of the chunk table");
    }
    if (table == &grown) {
        table_dev_.release();
        table_dev_ = grown;
        table_cap_ = cap;
    }
    table_rows_ = chunks_.size();
    return ok();
}

SearchError IndexBuilder::add(uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors, uint32_t vector_len,
                              bool on_device, hipStream_t stream, uint64_t* out_bad_row) {
    std::lock_guard<std::mutex> lock(mu_);
    if (spent_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the builder is finished: only destroy and record_count remain valid");
    if (vector_len != dim_)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "expected " + std::to_string(dim_) + ", found " + std::to_string(vector_len));
    if (n == 0) return ok();
    if (!doc_ids || !vectors) return make_error(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return add_locked(n, doc_ids, doc_id_lens, vectors, on_device, on_device ? stream : stream_, out_bad_row);
}

SearchError IndexBuilder::add_embedded(const std::function<SearchError(float*)>& embed, int embedder_device, uint32_t embedder_dim, uint32_t n,
                                       const char* const* doc_ids, const uint32_t* doc_id_lens, uint64_t* out_bad_row) {
    std::lock_guard<std::mutex> lock(mu_);
    if (spent_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the builder is finished: only destroy and record_count remain valid");
    if (embedder_device != device_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the embedder lives on another device than the builder");
    if (embedder_dim != dim_)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "expected " + std::to_string(dim_) + ", found " + std::to_string(embedder_dim));
    if (n == 0) return ok();
    if (!doc_ids) return make_error(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(embed_out_.reserve((size_t)n * dim_ * 4));
    FSGPU_TRY(embed(static_cast<float*>(embed_out_.ptr)));   // (complete when it returns: the embedders synchronise their stream)
    return add_locked(n, doc_ids, doc_id_lens, static_cast<const float*>(embed_out_.ptr), true, stream_, out_bad_row);
}

SearchError IndexBuilder::add_locked(uint64_t n, const char* const* doc_ids, const uint32_t* doc_id_lens, const float* vectors, bool on_device,
                                     hipStream_t stream, uint64_t* out_bad_row) {
    if (count_ + n >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row ids must fit in u32 (VectorHit.index)");
    for (uint64_t i = 0; i < n; ++i)
        if (!doc_ids[i]) return make_error(FSGPU_ERR_NULL_ARGUMENT, "doc id is null");
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(ensure_chunks(count_ + n));
    const uint64_t fit = kMaxLaunchElems / dim_;   // >= 8: dim <= 2^28
    const uint64_t slice = std::min<uint64_t>(on_device ? kBuildLaunchRows : kHostSliceRows, fit);
    if (!on_device) FSGPU_TRY(upload_.reserve((size_t)std::min(n, slice) * dim_ * 4));
    std::vector<uint32_t> lens((size_t)n);   // (before the enqueue: what can be allocated ahead of the device pass is)

    // ---- the device pass: enqueued whole, then the doc ids are checked while it runs ----
    const auto t0 = std::chrono::steady_clock::now();
    uint64_t launches = 0;
    hipError_t he = hipMemsetAsync(verdict_dev_.ptr, 0xff, 8, stream);
    if (he == hipSuccess) he = hipEventRecord(ev0_, stream);
    for (uint64_t r0 = 0; he == hipSuccess && r0 < n; r0 += slice) {
        const uint64_t rows = std::min(slice, n - r0);
        const float* src = vectors + (size_t)r0 * dim_;
        if (!on_device) {
            he = hipMemcpyAsync(upload_.ptr, src, (size_t)rows * dim_ * 4, hipMemcpyHostToDevice, stream);
            src = static_cast<const float*>(upload_.ptr);
            if (he != hipSuccess) break;
        }
        IngestArgs a;
        a.src = src;
        a.chunks = static_cast<unsigned char* const*>(table_dev_.ptr);
        a.chunk_rows = chunk_rows_;
        a.dim = dim_;
        a.n = (uint32_t)rows;
        a.to_f16 = opt_.quantization == 1 ? 1u : 0u;
        a.first_pos = count_ + r0;
        a.first_row = r0;
        a.verdict = static_cast<u64*>(verdict_dev_.ptr);
        he = launch_build_ingest(a, stream);
        ++launches;
    }
    if (he == hipSuccess) he = hipEventRecord(ev1_, stream);
    if (he == hipSuccess) he = hipMemcpyAsync(verdict_host_, verdict_dev_.ptr, 8, hipMemcpyDeviceToHost, stream);

    // (the duplicate rule allocates; if that throws, nothing of this call stays in flight behind the exception)
    uint64_t host_bad = ~0ull;
    const char* host_rule = nullptr;
    std::unordered_set<std::string> fresh;
    try {
        for (uint64_t i = 0; i < n; ++i) {
            const size_t len = doc_id_lens ? doc_id_lens[i] : std::strlen(doc_ids[i]);
            if (len > 0xffffu) {
                host_bad = i;
                host_rule = "doc_id byte length must fit in u16";
                break;
            }
            lens[(size_t)i] = (uint32_t)len;
            if (opt_.reject_duplicates) {
                std::string id(doc_ids[i], len);
                if (seen_.count(id) || !fresh.insert(std::move(id)).second) {
                    host_bad = i;
                    host_rule = "duplicate doc_id; each document must have a unique id";
                    break;
                }
            }
        }
    } catch (...) {
        (void)hipStreamSynchronize(stream);
        throw;
    }

    const hipError_t se = hipStreamSynchronize(stream);   // (also after a failed enqueue: nothing of this call stays in flight)
    if (he == hipSuccess) he = se;
    stats_.ingest_ms += ms_since(t0);
    stats_.ingest_launches += launches;
    if (he != hipSuccess) return hip_fail(he, "ingest of the rows");
    float dev_ms = 0.f;
    if (hipEventElapsedTime(&dev_ms, ev0_, ev1_) == hipSuccess) stats_.ingest_device_ms += dev_ms;

    // ---- the verdict: the first offending row of the call; of one row, write_record's order (vector before doc id) ----
    const uint64_t dv = *verdict_host_;
    const uint64_t dev_bad = dv == kBuildVerdictNone ? ~0ull : dv >> 8;
    if (dev_bad != ~0ull && dev_bad <= host_bad) {
        if (out_bad_row) *out_bad_row = dev_bad;
        return make_error(FSGPU_ERR_INVALID_CONFIG,
                          (dv & 0xff) == kBuildNonFinite
                              ? "all embedding values must be finite"
                              : "embedding norm must be non-zero and finite; a zero vector can never match any query");   // lib.rs:3651, :3658
    }
    if (host_bad != ~0ull) {
        if (out_bad_row) *out_bad_row = host_bad;
        return make_error(FSGPU_ERR_INVALID_CONFIG, host_rule);
    }

    // ---- admitted: FNV-1a now, the sort at finish ----
    uint64_t bytes = 0;
    for (uint64_t i = 0; i < n; ++i) bytes += lens[(size_t)i];
    // (room first, the duplicate set's buckets included, so that nothing below throws half way: the pushes fit, and merge() moves
    // the nodes of `fresh` (disjoint from seen_, as checked above) without allocating.  Doubling, so that a long series of adds does
    // not copy the tables every time)
    auto grow = [](auto& c, size_t need) {
        if (c.capacity() < need) c.reserve(std::max(need, c.capacity() * 2));
    };
    grow(hashes_, hashes_.size() + (size_t)n);
    grow(id_offsets_, id_offsets_.size() + (size_t)n);
    grow(id_blob_, id_blob_.size() + (size_t)bytes);
    seen_.reserve(seen_.size() + fresh.size());
    for (uint64_t i = 0; i < n; ++i) {
        hashes_.push_back(fnv1a(doc_ids[i], lens[(size_t)i]));
        id_blob_.append(doc_ids[i], lens[(size_t)i]);
        id_offsets_.push_back(id_blob_.size());
    }
    seen_.merge(fresh);
    count_ += n;
    return ok();
}

SearchError IndexBuilder::finish(const char* path, VectorIndex* out, Stats* stats) {
    std::lock_guard<std::mutex> lock(mu_);
    if (spent_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the builder is finished: only destroy and record_count remain valid");
    if (!out) return make_error(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    const uint64_t n = count_;
    if (id_blob_.size() > 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "string table exceeds u32 offsets");
    FSGPU_HIP(hipSetDevice(device_));
    Stats st = stats_;

    // ---- the order of the file: (hash, doc id bytes), equal keys in arrival order (lib.rs:3753-3762) ----
    auto t = std::chrono::steady_clock::now();
    struct Key {
        uint64_t hash;
        uint64_t seq;
    };
    std::vector<Key> keys((size_t)n);
    for (uint64_t i = 0; i < n; ++i) keys[(size_t)i] = Key{hashes_[(size_t)i], i};
    // (arrival position as the last key: the stable sort's result without its scratch copy)
    std::sort(keys.begin(), keys.end(), [&](const Key& a, const Key& b) {
        if (a.hash != b.hash) return a.hash < b.hash;
        const size_t al = (size_t)(id_offsets_[a.seq + 1] - id_offsets_[a.seq]), bl = (size_t)(id_offsets_[b.seq + 1] - id_offsets_[b.seq]);
        const int c = std::memcmp(id_blob_.data() + id_offsets_[a.seq], id_blob_.data() + id_offsets_[b.seq], std::min(al, bl));
        if (c != 0) return c < 0;
        if (al != bl) return al < bl;
        return a.seq < b.seq;
    });
    std::vector<uint32_t> perm((size_t)n);
    for (uint64_t i = 0; i < n; ++i) perm[(size_t)i] = (uint32_t)keys[(size_t)i].seq;
    st.sort_ms = ms_since(t);

    // ---- the slab: staged rows gathered into file order, device to device ----
    t = std::chrono::steady_clock::now();
    DeviceBuffer slab, perm_dev;
    auto release = [&]() {
        slab.release();
        perm_dev.release();
    };
    SearchError e = slab.reserve((size_t)n * row_bytes_);
    if (e.ok()) e = perm_dev.reserve((size_t)n * 4);
    if (!e.ok()) {
        release();
        return e;
    }
    hipError_t he = n ? hipMemcpyAsync(perm_dev.ptr, perm.data(), (size_t)n * 4, hipMemcpyHostToDevice, stream_) : hipSuccess;
    PermuteArgs pa;
    pa.chunks = static_cast<unsigned char* const*>(table_dev_.ptr);
    pa.chunk_rows = chunk_rows_;
    pa.row_bytes = row_bytes_;
    pa.perm = static_cast<const uint32_t*>(perm_dev.ptr);
    pa.out = static_cast<unsigned char*>(slab.ptr);
    if (he == hipSuccess) he = hipEventRecord(ev0_, stream_);
    for (uint64_t r0 = 0; he == hipSuccess && r0 < n; r0 += kBuildLaunchRows) {
        pa.row_begin = r0;
        pa.row_end = std::min<uint64_t>(r0 + kBuildLaunchRows, n);
        he = launch_build_permute(pa, stream_);
        ++st.permute_launches;
    }
    if (he == hipSuccess) he = hipEventRecord(ev1_, stream_);
    const hipError_t se = hipStreamSynchronize(stream_);
    if (he == hipSuccess) he = se;
    if (he != hipSuccess) {
        release();
        return hip_fail(he, "gather of the staged rows");
    }
    st.permute_ms = ms_since(t);
    float dev_ms = 0.f;
    if (hipEventElapsedTime(&dev_ms, ev0_, ev1_) == hipSuccess) st.permute_device_ms = dev_ms;
    st.rows = n;
    st.chunks = chunks_.size();
    st.peak_device_bytes = (uint64_t)chunks_.size() * chunk_rows_ * row_bytes_ + slab.bytes + perm_dev.bytes + table_dev_.bytes;
    perm_dev.release();

    // ---- the record table and the string table, in file order ----
    t = std::chrono::steady_clock::now();
    std::vector<uint64_t> hashes((size_t)n), offsets((size_t)n + 1);
    std::string blob;
    blob.reserve(id_blob_.size());
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t s = keys[(size_t)i].seq;
        hashes[(size_t)i] = keys[(size_t)i].hash;
        offsets[(size_t)i] = blob.size();
        blob.append(id_blob_, (size_t)id_offsets_[(size_t)s], (size_t)(id_offsets_[(size_t)s + 1] - id_offsets_[(size_t)s]));
    }
    offsets[(size_t)n] = blob.size();
    st.tables_ms = ms_since(t);

    if (path) {
        t = std::chrono::steady_clock::now();
        e = write_file(path, hashes, offsets, blob, slab);
        if (!e.ok()) {
            release();
            return e;
        }
        st.file_ms = ms_since(t);
    }

    e = out->adopt_built(device_, dim_, n, &slab, opt_.quantization == 0, &hashes, &offsets, &blob, embedder_id_, embedder_revision_,
                         opt_.compaction_gen);
    if (!e.ok()) {
        release();
        return e;
    }
    // ---- spent: the staging goes, the count stays ----
    release_staging();
    for (DeviceBuffer* b : {&upload_, &embed_out_}) b->release();
    std::vector<uint64_t>().swap(hashes_);
    std::vector<uint64_t>().swap(id_offsets_);
    std::string().swap(id_blob_);
    seen_.clear();
    spent_ = true;
    stats_ = st;
    if (stats) *stats = st;
    return ok();
}

// header | 16-byte records | string table | pad to 64 | slab (lib.rs:3764-3943, header :5714-5768), to `path`.tmp and renamed over
// `path` (as VectorIndex::rewrite writes its image); the slab comes down in blocks of 64 MiB
SearchError IndexBuilder::write_file(const char* path, const std::vector<uint64_t>& hashes, const std::vector<uint64_t>& offsets,
                                     const std::string& blob, const DeviceBuffer& slab) const {
    const uint64_t n = hashes.size();
    const size_t idl = embedder_id_.size(), rvl = embedder_revision_.size();
    const size_t header_len = 4 + 2 + 2 + idl + 2 + rvl + 4 + 1 + 3 + 8 + 8 + 4;
    const uint64_t pre = (uint64_t)header_len + n * 16 + blob.size();
    const uint64_t vectors_offset = (pre + 63) / 64 * 64;
    const uint64_t slab_bytes = n * row_bytes_;
    std::vector<uint8_t> head((size_t)vectors_offset, 0);
    auto put = [&](size_t at, uint64_t v, int bytes) {
        for (int b = 0; b < bytes; ++b) head[at + b] = (uint8_t)(v >> (8 * b));
    };
    size_t c = 0;
    std::memcpy(head.data(), "FSVI", 4);
    c += 4;
    put(c, 1, 2);
    c += 2;
    for (const std::string* s : {&embedder_id_, &embedder_revision_}) {
        put(c, s->size(), 2);
        c += 2;
        std::memcpy(head.data() + c, s->data(), s->size());
        c += s->size();
    }
    put(c, dim_, 4);
    c += 4;
    head[c++] = opt_.quantization;
    head[c++] = opt_.compaction_gen;
    put(c, 0, 2);   // publication nonce: 0, as fsgpu_fsvi_write writes it
    c += 2;
    put(c, n, 8);
    c += 8;
    put(c, vectors_offset, 8);
    c += 8;
    put(c, crc32_ieee(head.data(), c), 4);
    c += 4;
    for (uint64_t i = 0; i < n; ++i) {
        put(c + (size_t)i * 16, hashes[(size_t)i], 8);
        put(c + (size_t)i * 16 + 8, offsets[(size_t)i], 4);
        put(c + (size_t)i * 16 + 12, offsets[(size_t)i + 1] - offsets[(size_t)i], 2);
    }
    std::memcpy(head.data() + c + (size_t)n * 16, blob.data(), blob.size());
    const std::string tmp = std::string(path) + ".tmp";
    SearchError fe = ok();
    FILE* f = std::fopen(tmp.c_str(), "wb");
    if (!f) fe = make_error(FSGPU_ERR_IO, "cannot create " + tmp);
    if (fe.ok() && std::fwrite(head.data(), 1, head.size(), f) != head.size()) fe = make_error(FSGPU_ERR_IO, "short write to " + tmp);
    std::vector<uint8_t> block;
    const uint64_t kBlock = 64ull << 20;
    for (uint64_t b0 = 0; fe.ok() && b0 < slab_bytes; b0 += kBlock) {
        const size_t nb = (size_t)std::min(kBlock, slab_bytes - b0);
        block.resize(nb);
        const hipError_t he = hipMemcpy(block.data(), static_cast<const unsigned char*>(slab.ptr) + b0, nb, hipMemcpyDeviceToHost);
        if (he != hipSuccess) fe = hip_fail(he, "download of the slab");
        else if (std::fwrite(block.data(), 1, nb, f) != nb) fe = make_error(FSGPU_ERR_IO, "short write to " + tmp);
    }
    if (f) {
        if (fe.ok() && (std::fflush(f) != 0 || fsync(fileno(f)) != 0)) fe = make_error(FSGPU_ERR_IO, "cannot flush " + tmp);
        std::fclose(f);
    }
    if (fe.ok() && std::rename(tmp.c_str(), path) != 0) fe = make_error(FSGPU_ERR_IO, std::string("cannot rename over ") + path);
    if (!fe.ok() && f) std::remove(tmp.c_str());
    return fe;
}

}  // namespace fsgpu

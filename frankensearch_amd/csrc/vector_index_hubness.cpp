// vector_index_hubness.cpp — compute_query_hubness (crates/frankensearch-fusion/src/hubness.rs:109-138) over every row of a
// VectorIndex: the kernel of hubness_kernels.hip, launched over row ranges, and the host restatement (hubness.hpp) on rows fetched
// from the slab in blocks for the shapes the kernel does not take.  The same bits either way.
#include "hubness.hpp"
#include "mmr.hpp"
#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

SearchError VectorIndex::compute_query_hubness(const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq, float* out,
                                               float* out_topk) {
    if (catalog_only_ || (!slab_dev_ && nrows_ > 0)) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (nq > 0 && query_dim != dim_)   // stricter than the reference's truncation to the common length (hubness.rs:157-161)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "query sample has dimension " + std::to_string(query_dim) + ", the index " +
                                                            std::to_string(dim_));
    if (nq == 0 || kq == 0) {   // hubness.rs:110-112
        for (uint64_t r = 0; r < nrows_; ++r) out[r] = 0.0f;
        return ok();
    }
    if (nrows_ == 0) return ok();
    const uint32_t k = std::min(kq, nq);
    const size_t stride = row_stride_ ? row_stride_ : (size_t)dim_ * (f32_ ? 4 : 2);
    FSGPU_HIP(hipSetDevice(device_));
    if (k > kHubMaxK || dim_ > kHubMaxDim) {
        // the host restatement over blocks of rows copied up from the slab
        const uint64_t block = std::max<uint64_t>(1, std::min<uint64_t>(nrows_, (8u << 20) / ((size_t)dim_ * 4)));
        std::vector<unsigned char> raw(block * (size_t)dim_ * (f32_ ? 4 : 2));
        std::vector<float> wide(f32_ ? 0 : block * (size_t)dim_);
        std::vector<const float*> docs(block), qptr(nq);
        std::vector<uint32_t> doc_lens(block, dim_), q_lens(nq, dim_);
        for (uint32_t j = 0; j < nq; ++j) qptr[j] = queries + (size_t)j * dim_;
        const size_t row_bytes = (size_t)dim_ * (f32_ ? 4 : 2);
        for (uint64_t r0 = 0; r0 < nrows_; r0 += block) {
            const uint64_t n = std::min(block, nrows_ - r0);
            const unsigned char* src = static_cast<const unsigned char*>(slab_dev_) + r0 * stride;
            FSGPU_HIP(hipMemcpy2D(raw.data(), row_bytes, src, stride, row_bytes, n, hipMemcpyDeviceToHost));
            const float* base = reinterpret_cast<const float*>(raw.data());
            if (!f32_) {
                const uint16_t* h = reinterpret_cast<const uint16_t*>(raw.data());
                for (size_t i = 0; i < n * (size_t)dim_; ++i) wide[i] = f16_bits_to_f32(h[i]);
                base = wide.data();
            }
            for (uint64_t i = 0; i < n; ++i) docs[i] = base + i * (size_t)dim_;
            query_hubness_host(docs.data(), doc_lens.data(), n, qptr.data(), q_lens.data(), nq, kq, hreduce, out + r0,
                               out_topk ? out_topk + r0 * k : nullptr);
        }
        return ok();
    }
    // workspaces of this call's own (the searches' are untouched), ordered on the index's stream
    const size_t q_bytes = (size_t)nq * dim_ * 4;
    FSGPU_TRY(ws_hub_q_.reserve(q_bytes));
    FSGPU_TRY(ws_hub_out_.reserve((size_t)nrows_ * 4));
    if (out_topk) FSGPU_TRY(ws_hub_topk_.reserve((size_t)nrows_ * k * 4));
    FSGPU_HIP(hipMemcpyAsync(ws_hub_q_.ptr, queries, q_bytes, hipMemcpyHostToDevice, stream_));
    HubnessArgs a{};
    a.slab = slab_dev_;
    a.row_stride = (uint32_t)stride;
    a.dim = dim_;
    a.slab_f32 = f32_ ? 1u : 0u;
    a.queries = static_cast<const float*>(ws_hub_q_.ptr);
    a.nq = nq;
    a.k = k;
    a.hreduce = hreduce;
    a.out = static_cast<float*>(ws_hub_out_.ptr);
    a.out_topk = out_topk ? static_cast<float*>(ws_hub_topk_.ptr) : nullptr;
    for (uint64_t r0 = 0; r0 < nrows_; r0 += kHubLaunchRows) {
        a.row0 = (uint32_t)r0;
        a.nrows = (uint32_t)std::min<uint64_t>(kHubLaunchRows, nrows_ - r0);
        FSGPU_HIP(launch_hubness(a, stream_));
    }
    FSGPU_HIP(hipMemcpyAsync(out, ws_hub_out_.ptr, (size_t)nrows_ * 4, hipMemcpyDeviceToHost, stream_));
    if (out_topk) FSGPU_HIP(hipMemcpyAsync(out_topk, ws_hub_topk_.ptr, (size_t)nrows_ * k * 4, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    return ok();
}

}  // namespace fsgpu

// vector_index_mmr.cpp — Maximum Marginal Relevance over rows of a VectorIndex (mmr_kernels.hip) and the row accessor it falls
// back on: vector_at_f32, mmr_rerank_rows (pools as global row ids, one launch for a batch), mmr_rerank_docs (the searcher's stage:
// doc ids resolved through the WAL and the record table).  The arithmetic is the reference's mmr_rerank
// (crates/frankensearch-fusion/src/mmr.rs:103-319); mmr.hpp holds its host restatement.
#include "mmr.hpp"
#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

SearchError VectorIndex::vector_at_f32(uint32_t row, float* out) {
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (row < row_base_ || row - row_base_ >= nrows_)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "row index " + std::to_string(row) + " out of range for vector_at_f32 (" +
                                                        std::to_string(nrows_) + " records)");
    FSGPU_HIP(hipSetDevice(device_));
    const size_t stride = row_stride_ ? row_stride_ : (size_t)dim_ * (f32_ ? 4 : 2);   // (0 = dense rows; set on MRL prefix views)
    const unsigned char* src = static_cast<const unsigned char*>(slab_dev_) + (size_t)(row - row_base_) * stride;
    if (f32_) {
        FSGPU_HIP(hipMemcpy(out, src, (size_t)dim_ * 4, hipMemcpyDeviceToHost));
        return ok();
    }
    std::vector<uint16_t> half(dim_);
    FSGPU_HIP(hipMemcpy(half.data(), src, (size_t)dim_ * 2, hipMemcpyDeviceToHost));
    for (uint32_t e = 0; e < dim_; ++e) out[e] = f16_bits_to_f32(half[e]);
    return ok();
}

SearchError VectorIndex::mmr_rerank_rows(const uint32_t* rows, const double* scores, const uint32_t* offsets, uint32_t nq, uint32_t k,
                                         double lambda, uint32_t candidate_pool, const int32_t* ovr_index, const float* ovr_vectors,
                                         uint32_t n_ovr, uint32_t* out_order, uint32_t* out_counts, double* out_sims) {
    if (nq == 0) return ok();
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    if (out_sims && nq != 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "the similarity matrix is returned for a single pool only");
    if (offsets[0] != 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "offsets[0] must be 0");
    for (uint32_t q = 0; q < nq; ++q)
        if (offsets[q + 1] < offsets[q]) return make_error(FSGPU_ERR_INVALID_CONFIG, "offsets must not decrease");
    const uint32_t total = offsets[nq];
    for (uint32_t i = 0; i < total; ++i) {
        if (ovr_index && ovr_index[i] >= 0) {
            if ((uint32_t)ovr_index[i] >= n_ovr) return make_error(FSGPU_ERR_INVALID_CONFIG, "override index out of range");
        } else if (rows[i] < row_base_ || rows[i] - row_base_ >= nrows_) {
            return make_error(FSGPU_ERR_INVALID_CONFIG, "row index " + std::to_string(rows[i]) + " out of range for vector_at_f32 (" +
                                                            std::to_string(nrows_) + " records)");
        }
    }
    lambda = mmr_clamped_lambda(lambda);
    // what the kernel takes, what the host restatement takes
    uint32_t max_n = 0, host_pools = 0;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t n = std::min(offsets[q + 1] - offsets[q], candidate_pool);
        if (n == 0 || k == 0) continue;
        if (mmr_device_pool(n, dim_)) max_n = std::max(max_n, n);
        else ++host_pools;
    }
    if (max_n > 0) {
        FSGPU_HIP(hipSetDevice(device_));
        const bool f32_staging = f32_ || n_ovr > 0;
        const MmrPlan plan = mmr_plan(max_n, dim_, f32_staging, out_sims != nullptr);
        // one block down: scores | rows | offsets | override indexes | override vectors
        const size_t o_scores = 0, o_rows = o_scores + (size_t)total * 8, o_offsets = o_rows + (size_t)total * 4,
                     o_ovr = o_offsets + (size_t)(nq + 1) * 4, o_ovec = (o_ovr + (n_ovr ? (size_t)total * 4 : 0) + 15) & ~(size_t)15,
                     in_bytes = o_ovec + (size_t)n_ovr * dim_ * 4;
        std::vector<unsigned char> in(in_bytes);
        std::memcpy(in.data() + o_scores, scores, (size_t)total * 8);
        std::memcpy(in.data() + o_rows, rows, (size_t)total * 4);
        std::memcpy(in.data() + o_offsets, offsets, (size_t)(nq + 1) * 4);
        if (n_ovr) {
            std::memcpy(in.data() + o_ovr, ovr_index, (size_t)total * 4);
            std::memcpy(in.data() + o_ovec, ovr_vectors, (size_t)n_ovr * dim_ * 4);
        }
        const size_t out_bytes = ((size_t)total + nq) * 4;
        FSGPU_TRY(ws_mmr_in_.reserve(in_bytes));
        FSGPU_TRY(ws_mmr_out_.reserve(out_bytes));
        if (plan.sims_global) FSGPU_TRY(ws_mmr_sims_.reserve((size_t)total * max_n * 8));
        if (plan.storage == kMmrStageGlobalF32) FSGPU_TRY(ws_mmr_vec_.reserve((size_t)total * plan.vec_stride * 4));
        unsigned char* in_dev = static_cast<unsigned char*>(ws_mmr_in_.ptr);
        FSGPU_HIP(hipMemcpyAsync(in_dev, in.data(), in_bytes, hipMemcpyHostToDevice, stream_));
        MmrArgs a{};
        a.slab = slab_dev_;
        a.row_base = row_base_;
        a.row_stride = row_stride_ ? row_stride_ : dim_ * (f32_ ? 4 : 2);
        a.dim = dim_;
        a.slab_f32 = f32_ ? 1u : 0u;
        a.k = k;
        a.candidate_pool = candidate_pool;
        a.lambda = lambda;
        a.scores = reinterpret_cast<const double*>(in_dev + o_scores);
        a.rows = reinterpret_cast<const uint32_t*>(in_dev + o_rows);
        a.offsets = reinterpret_cast<const uint32_t*>(in_dev + o_offsets);
        a.ovr_index = n_ovr ? reinterpret_cast<const int32_t*>(in_dev + o_ovr) : nullptr;
        a.ovr_vectors = n_ovr ? reinterpret_cast<const float*>(in_dev + o_ovec) : nullptr;
        a.out_order = static_cast<uint32_t*>(ws_mmr_out_.ptr);
        a.out_counts = a.out_order + total;
        a.sims = plan.sims_global ? static_cast<double*>(ws_mmr_sims_.ptr) : nullptr;
        a.sim_pitch = max_n;
        a.lds_sims_offset = plan.lds_sims_offset;
        a.vec_ws = plan.storage == kMmrStageGlobalF32 ? static_cast<float*>(ws_mmr_vec_.ptr) : nullptr;
        a.vec_stride = plan.vec_stride;
        FSGPU_HIP(launch_mmr(a, nq, plan, stream_));
        std::vector<uint32_t> out((size_t)total + nq);
        FSGPU_HIP(hipMemcpyAsync(out.data(), ws_mmr_out_.ptr, out_bytes, hipMemcpyDeviceToHost, stream_));
        if (out_sims) {
            const uint32_t n = std::min(total, candidate_pool);
            if (mmr_device_pool(n, dim_) && k > 0)
                FSGPU_HIP(hipMemcpyAsync(out_sims, ws_mmr_sims_.ptr, (size_t)n * n * 8, hipMemcpyDeviceToHost, stream_));
        }
        FSGPU_HIP(hipStreamSynchronize(stream_));
        for (uint32_t q = 0; q < nq; ++q) {
            const uint32_t n = std::min(offsets[q + 1] - offsets[q], candidate_pool);
            if (n == 0 || k == 0) {
                out_counts[q] = 0;
            } else if (mmr_device_pool(n, dim_)) {
                out_counts[q] = out[total + q];
                std::memcpy(out_order + offsets[q], out.data() + offsets[q], (size_t)out_counts[q] * 4);
            }
        }
    }
    if (max_n == 0 && host_pools == 0) {
        for (uint32_t q = 0; q < nq; ++q) out_counts[q] = 0;
        return ok();
    }
    if (host_pools == 0) return ok();
    // pools past the kernel's limits: mmr_rerank_host on vectors fetched from the slab (vector_at_f32) or taken from the overrides
    std::vector<float> store;
    std::vector<const float*> ptrs;
    std::vector<uint32_t> lens;
    for (uint32_t q = 0; q < nq; ++q) {
        const uint32_t begin = offsets[q], n = std::min(offsets[q + 1] - begin, candidate_pool);
        if (n == 0 || k == 0) {
            out_counts[q] = 0;
            continue;
        }
        if (mmr_device_pool(n, dim_)) continue;
        store.assign((size_t)n * dim_, 0.0f);
        ptrs.assign(n, nullptr);
        lens.assign(n, dim_);
        for (uint32_t i = 0; i < n; ++i) {
            if (ovr_index && ovr_index[begin + i] >= 0) {
                ptrs[i] = ovr_vectors + (size_t)ovr_index[begin + i] * dim_;
            } else {
                FSGPU_TRY(vector_at_f32(rows[begin + i], store.data() + (size_t)i * dim_));
                ptrs[i] = store.data() + (size_t)i * dim_;
            }
        }
        mmr_rerank_host(scores + begin, ptrs.data(), lens.data(), n, k, lambda, candidate_pool, out_order + begin, out_counts + q, out_sims);
    }
    return ok();
}

SearchError VectorIndex::mmr_rerank_docs(const char* const* doc_ids, const uint32_t* doc_id_lens, const float* scores, uint32_t n,
                                         bool enabled, double lambda, uint32_t candidate_pool, uint32_t* out_order, uint8_t* out_applied) {
    *out_applied = 0;
    for (uint32_t i = 0; i < n; ++i) out_order[i] = i;
    if (!enabled || n < 2) return ok();   // searcher.rs:2698
    const uint32_t pool = std::min(n, std::max(candidate_pool, 1u));
    if (pool < 2) return ok();
    if (doc_offsets_.empty()) return make_error(FSGPU_ERR_INVALID_CONFIG, "index has no doc-id table");
    std::vector<uint32_t> rows(pool, 0), order(pool);
    std::vector<int32_t> ovr(pool, -1);
    std::vector<double> wide(pool);
    std::vector<float> ovr_vectors;
    uint32_t n_ovr = 0;
    for (uint32_t i = 0; i < pool; ++i) {
        const int64_t w = wal_latest(doc_ids[i], doc_id_lens[i]);
        if (w >= 0) {   // the newest WAL entry of the document wins (two_tier.rs:1858-1863)
            const std::vector<float>& v = wal_[(size_t)w].embedding;
            ovr_vectors.insert(ovr_vectors.end(), v.begin(), v.end());
            ovr[i] = (int32_t)n_ovr++;
        } else {
            const int64_t r = find_index_by_doc_id(doc_ids[i], doc_id_lens[i]);
            if (r < 0) return ok();   // incomplete pool: the results stay as they are (searcher.rs:2705-2717)
            rows[i] = (uint32_t)(row_base_ + (uint64_t)r);
        }
        wide[i] = (double)scores[i];
    }
    const uint32_t offsets[2] = {0, pool};
    uint32_t count = 0;
    FSGPU_TRY(mmr_rerank_rows(rows.data(), wide.data(), offsets, 1, pool, lambda, candidate_pool, n_ovr ? ovr.data() : nullptr,
                              ovr_vectors.data(), n_ovr, order.data(), &count, nullptr));
    if (count != pool) return ok();   // `order.len() == pool` (searcher.rs:2726)
    std::memcpy(out_order, order.data(), (size_t)pool * 4);
    *out_applied = 1;
    return ok();
}

}  // namespace fsgpu

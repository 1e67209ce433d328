// hubness.hpp — the host restatement of the reference's query-hubness table build (crates/frankensearch-fusion/src/hubness.rs:
// compute_query_hubness :109-126, doc_hubness :130-138, dot :158-161), defined in fusion.cpp.  It needs no device: it is
// fsgpu_query_hubness, the answer for shapes the kernel does not take (k > 64, dim > 1,024) and the comparator of the device path —
// the same bits either way.
#pragma once

#include <cstdint>
#include <cstring>

namespace fsgpu {

// f32::total_cmp as an unsigned key (larger = greater): -NaN < -inf < ... < -0.0 < +0.0 < ... < +inf < +NaN.  NOT the scan's
// score_ord, which ranks every NaN as -inf (search.rs score_key); hubness.rs:135 selects with a bare total_cmp.
inline uint32_t hubness_key(float x) {
    uint32_t b;
    std::memcpy(&b, &x, 4);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
inline float hubness_value(uint32_t key) {
    const uint32_t b = (key & 0x80000000u) ? (key & 0x7fffffffu) : ~key;
    float x;
    std::memcpy(&x, &b, 4);
    return x;
}

// dot_product_f32_f32 (crates/frankensearch-index/src/simd.rs:134-222) in the index's horizontal order: four 8-lane accumulators
// over groups of 32, (acc0 + acc1) + (acc2 + acc3), leftover chunks added to that sum, reduce_add, unfused tail
float hubness_dot(const float* a, const float* b, size_t n, int hreduce);

// The mean of the k greatest keys in the project's canonical order (hubness.rs:136-137 leaves the order of `top` open):
// v_1 >= ... >= v_k under total_cmp; s = v_1; s += v_2 .. v_{k-1}; (v_k + s) / k.  keys_desc holds k keys, greatest first.
float hubness_mean(const uint32_t* keys_desc, uint32_t k);

// out[d] for docs [0, n_docs); docs[d] holds doc_lens[d] values, queries[j] query_lens[j]; each dot runs over the common prefix
// (hubness.rs:157-161).  out_topk (nullable): the k = min(kq, n_queries) selected sims of every doc, greatest first, [n_docs, k].
// threads 0 = from OMP_NUM_THREADS, capped at 16.
void query_hubness_host(const float* const* docs, const uint32_t* doc_lens, uint64_t n_docs, const float* const* queries,
                        const uint32_t* query_lens, uint32_t n_queries, uint32_t kq, int hreduce, float* out, float* out_topk,
                        uint32_t threads = 0);

}  // namespace fsgpu

// mmr.hpp — the host restatement of the reference's mmr_rerank (crates/frankensearch-fusion/src/mmr.rs:103-319), defined in
// fusion.cpp.  It needs no device: it is fsgpu_mmr_rerank, the answer for pools the kernel does not take (larger than
// mmr_device_pool, or ragged) and the comparator of the device path — the same bits either way.
#pragma once

#include <cstdint>
#include <cstring>
#include <vector>

namespace fsgpu {

// MmrConfig::clamped_lambda (mmr.rs:72-83): non-finite or negative -> 0, above 1 -> 1
double mmr_clamped_lambda(double lambda);

// scores[n], vectors[n] of lengths[n] f32 values each.  out_order holds min(k, min(n, candidate_pool)) entries, *out_count the
// number selected; out_sims (optional) is the pool x pool matrix of sim(i, j) as the selection reads it.
void mmr_rerank_host(const double* scores, const float* const* vectors, const uint32_t* lengths, uint32_t n, uint32_t k, double lambda,
                     uint32_t candidate_pool, uint32_t* out_order, uint32_t* out_count, double* out_sims);

// IEEE binary16 bits widened to f32 (exact; what vector_at_f32 returns for an F16 slab)
inline float f16_bits_to_f32(uint16_t h) {
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
    if (exp == 0x1fu) {
        bits = sign | 0x7f800000u | (man << 13);
    } else if (exp != 0) {
        bits = sign | ((exp + 112u) << 23) | (man << 13);
    } else if (man == 0) {
        bits = sign;
    } else {   // subnormal: normalise
        int shift = 0;
        while (!(man & 0x400u)) man <<= 1, ++shift;
        bits = sign | ((uint32_t)(113 - shift) << 23) | ((man & 0x3ffu) << 13);
    }
    float f;
    std::memcpy(&f, &bits, 4);
    return f;
}

}  // namespace fsgpu

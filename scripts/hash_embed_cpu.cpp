// hash_embed_cpu.cpp — the CPU yardstick of scripts/bench_hash_embed.py: a C++ restatement of the reference's HashEmbedder
// (crates/frankensearch-embed/src/hash_embedder.rs) for ASCII texts, spread over a given number of threads as embed_batch_sync
// spreads a batch over rayon (:254-260).  Not part of the product: it exists because the Rust cannot be built where the bench runs.
//   tokenize :627-659 (the ASCII path), fnv1a_hash :588-595, embed_fnv_modular :263-280,
//   embed_jl :299-327 with jl_accumulate_lanes8_scalar :467-481 (groups of 8 chains, 8 - 2 * odd) and jl_accumulate_one :339-346,
//   l2_normalize_in_place core/src/traits.rs:606-618.
// Built by the script with -O3 -march=native, so the 8-chain loop is vectorised as the reference's AVX2 form is.
#include <cmath>
#include <cstdint>
#include <cstring>
#include <thread>
#include <vector>

namespace {

inline bool alnum(uint8_t b) { return (uint8_t)(b - '0') < 10 || (uint8_t)((b | 0x20) - 'a') < 26; }

inline void xorshift(uint64_t& s) {
    s ^= s << 13;
    s ^= s >> 7;
    s ^= s << 17;
}

void embed_one(const uint8_t* p, const uint8_t* end, uint32_t dim, int jl, uint64_t seed, float* e) {
    std::memset(e, 0, (size_t)dim * 4);
    uint64_t states[8];
    int filled = 0;
    while (p < end) {
        while (p < end && !alnum(*p)) ++p;
        const uint8_t* start = p;
        uint64_t h = 0xcbf29ce484222325ull;
        while (p < end && alnum(*p)) h = (h ^ *p++) * 0x100000001b3ull;
        if (p - start < 2) continue;
        if (!jl) {
            e[h % dim] += (h >> 63) == 1 ? 1.0f : -1.0f;
            continue;
        }
        states[filled++] = (seed ^ h) | 1;
        if (filled == 8) {
            uint64_t s[8];
            std::memcpy(s, states, sizeof s);
            for (uint32_t d = 0; d < dim; ++d) {
                int odd = 0;
                for (int i = 0; i < 8; ++i) {
                    xorshift(s[i]);
                    odd += (int)(s[i] & 1);
                }
                e[d] += (float)(8 - 2 * odd);
            }
            filled = 0;
        }
    }
    for (int i = 0; i < filled; ++i) {
        uint64_t s = states[i];
        for (uint32_t d = 0; d < dim; ++d) {
            xorshift(s);
            e[d] += (s & 1) == 0 ? 1.0f : -1.0f;
        }
    }
    float norm_sq = 0.f;
    for (uint32_t d = 0; d < dim; ++d) norm_sq += e[d] * e[d];
    if (!std::isfinite(norm_sq) || norm_sq < 1.1920929e-7f) {
        std::memset(e, 0, (size_t)dim * 4);
        return;
    }
    const float inv = 1.0f / std::sqrt(norm_sq);
    for (uint32_t d = 0; d < dim; ++d) e[d] *= inv;
}

}  // namespace

extern "C" void hash_embed_cpu(const uint8_t* text, const uint32_t* offsets, uint32_t n, uint32_t dim, int jl, uint64_t seed, float* out,
                               uint32_t threads) {
    if (threads == 0) threads = 1;
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < threads; ++t)
        pool.emplace_back([=] {
            for (uint32_t i = t; i < n; i += threads) embed_one(text + offsets[i], text + offsets[i + 1], dim, jl, seed, out + (size_t)i * dim);
        });
    for (auto& th : pool) th.join();
}

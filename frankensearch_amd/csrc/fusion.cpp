// fusion.cpp — host-side rank fusion used after the GPU searches: reciprocal-rank fusion and the two-tier
// score blend.  O(k) work on a few hundred hits, so it stays on the CPU exactly as in the reference:
//   rrf_fuse        crates/frankensearch-fusion/src/rrf.rs:368-560 (cmp_for_ranking :179-198, sanitisers :85-138)
//   blend_two_tier  crates/frankensearch-fusion/src/blend.rs:107-195 (NormBounds :24-75, sanitisers :518-532)
// Exposed through the C ABI (fsgpu_rrf_fuse / fsgpu_blend_two_tier) so the end-to-end two-tier query path can be
// driven without the Rust crate.  No GPU needed.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <limits>
#include <new>
#include <string_view>
#include <thread>
#include <unordered_map>
#include <vector>

#include "../../include/fsgpu.h"
#include "hubness.hpp"
#include "mmr.hpp"

namespace {

constexpr double kDefaultRrfK = 60.0;

inline int32_t total_key32(float x) {
    int32_t b;
    std::memcpy(&b, &x, 4);
    return b ^ (int32_t)(((uint32_t)(b >> 31)) >> 1);
}
inline int64_t total_key64(double x) {
    int64_t b;
    std::memcpy(&b, &x, 8);
    return b ^ (int64_t)(((uint64_t)(b >> 63)) >> 1);
}
inline uint64_t fnv1a(std::string_view s) {
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : s) {
        h ^= c;
        h *= 0x100000001b3ull;
    }
    return h;
}
inline std::string_view sv(const fsgpu_scored_doc& d) { return std::string_view(d.doc_id, d.doc_id_len); }

struct Scratch {
    std::string_view doc;
    double rrf = 0.0;
    int64_t lexical_rank = -1, semantic_rank = -1;
    uint32_t semantic_index = 0;
    bool has_index = false;
    float lexical_score = 0.f, semantic_score = 0.f;
    bool in_both = false;
};

}  // namespace

extern "C" fsgpu_status fsgpu_rrf_fuse(const fsgpu_scored_doc* lexical, uint32_t n_lexical,
                                        const fsgpu_scored_doc* semantic, uint32_t n_semantic, double k,
                                        double lexical_weight, double semantic_weight, int32_t tiebreak, uint32_t limit,
                                        uint32_t offset, fsgpu_fused_hit* out, uint32_t* out_count) {
    if (!out_count || (n_lexical && !lexical) || (n_semantic && !semantic) || (limit && !out)) return FSGPU_ERR_NULL_ARGUMENT;
    *out_count = 0;
    if (!(std::isfinite(k) && k >= 0.0)) k = kDefaultRrfK;
    if (!(std::isfinite(lexical_weight) && lexical_weight > 0.0)) lexical_weight = 1.0;
    if (!(std::isfinite(semantic_weight) && semantic_weight > 0.0)) semantic_weight = 1.0;
    std::unordered_map<std::string_view, size_t> slot;
    std::vector<Scratch> hits;
    hits.reserve(((size_t)n_lexical + n_semantic) * 3 / 4 + 1);
    for (uint32_t rank = 0; rank < n_lexical; ++rank) {
        const double c = (1.0 / (k + (double)rank + 1.0)) * lexical_weight;
        auto it = slot.find(sv(lexical[rank]));
        if (it == slot.end()) {
            Scratch s;
            s.doc = sv(lexical[rank]);
            s.rrf = c;
            s.lexical_rank = rank;
            s.lexical_score = lexical[rank].score;
            slot.emplace(s.doc, hits.size());
            hits.push_back(s);
        } else {
            Scratch& h = hits[it->second];
            if (h.lexical_rank >= 0) continue;  // first (best) occurrence wins
            h.rrf += c;
            h.lexical_rank = rank;
            h.lexical_score = lexical[rank].score;
            if (h.semantic_rank >= 0) h.in_both = true;
        }
    }
    for (uint32_t rank = 0; rank < n_semantic; ++rank) {
        const double c = (1.0 / (k + (double)rank + 1.0)) * semantic_weight;
        auto it = slot.find(sv(semantic[rank]));
        if (it == slot.end()) {
            Scratch s;
            s.doc = sv(semantic[rank]);
            s.rrf = c;
            s.semantic_rank = rank;
            s.semantic_score = semantic[rank].score;
            s.semantic_index = semantic[rank].index;
            s.has_index = true;
            slot.emplace(s.doc, hits.size());
            hits.push_back(s);
        } else {
            Scratch& h = hits[it->second];
            if (h.semantic_rank >= 0) continue;
            h.rrf += c;
            h.semantic_rank = rank;
            h.semantic_score = semantic[rank].score;
            h.semantic_index = semantic[rank].index;
            h.has_index = true;
            if (h.lexical_rank >= 0) h.in_both = true;
        }
    }
    const size_t window = (size_t)limit + offset;
    if (window == 0) return FSGPU_OK;
    const bool hash_tiebreak = tiebreak == FSGPU_RRF_TIEBREAK_HASH;
    auto before = [&](const Scratch& a, const Scratch& b) {
        const int64_t ka = total_key64(a.rrf), kb = total_key64(b.rrf);
        if (ka != kb) return ka > kb;
        if (a.in_both != b.in_both) return a.in_both;
        if (hash_tiebreak) {
            const uint64_t ha = fnv1a(a.doc), hb = fnv1a(b.doc);
            if (ha != hb) return ha < hb;
        } else {
            const float la = a.lexical_rank >= 0 ? a.lexical_score : -std::numeric_limits<float>::infinity();
            const float lb = b.lexical_rank >= 0 ? b.lexical_score : -std::numeric_limits<float>::infinity();
            const int32_t x = total_key32(la), y = total_key32(lb);
            if (x != y) return x > y;
        }
        return a.doc < b.doc;
    };
    if (window < hits.size()) {
        std::nth_element(hits.begin(), hits.begin() + (window - 1), hits.end(), before);
        hits.resize(window);
    }
    std::sort(hits.begin(), hits.end(), before);
    uint32_t n = 0;
    for (size_t i = offset; i < hits.size() && n < limit; ++i, ++n) {
        const Scratch& h = hits[i];
        fsgpu_fused_hit& o = out[n];
        o.doc_id = h.doc.data();
        o.doc_id_len = (uint32_t)h.doc.size();
        o.rrf_score = h.rrf;
        o.lexical_rank = h.lexical_rank;
        o.semantic_rank = h.semantic_rank;
        o.semantic_index = h.has_index ? h.semantic_index : 0xffffffffu;
        o.lexical_score = h.lexical_score;
        o.semantic_score = h.semantic_score;
        o.in_both_sources = h.in_both ? 1 : 0;
    }
    *out_count = n;
    return FSGPU_OK;
}

extern "C" fsgpu_status fsgpu_blend_two_tier(const fsgpu_scored_doc* fast, uint32_t n_fast,
                                              const fsgpu_scored_doc* quality, uint32_t n_quality, float blend_factor,
                                              fsgpu_scored_doc* out, uint32_t* out_count) {
    if (!out_count || (n_fast && !fast) || (n_quality && !quality) || ((n_fast || n_quality) && !out))
        return FSGPU_ERR_NULL_ARGUMENT;
    *out_count = 0;
    const float alpha = std::isfinite(blend_factor) ? std::min(std::max(blend_factor, 0.0f), 1.0f) : 0.7f;
    struct Bounds {
        float min = std::numeric_limits<float>::infinity(), range = 0.f;
        bool saw = false;
    };
    auto bounds = [](const fsgpu_scored_doc* hits, uint32_t n) {
        Bounds b;
        float mx = -std::numeric_limits<float>::infinity();
        for (uint32_t i = 0; i < n; ++i)
            if (std::isfinite(hits[i].score)) {
                b.min = std::min(b.min, hits[i].score);
                mx = std::max(mx, hits[i].score);
                b.saw = true;
            }
        b.range = mx - b.min;
        return b;
    };
    auto apply = [](const Bounds& b, float s) {
        if (!b.saw || !std::isfinite(s)) return 0.0f;
        const float v = b.range > 1.1920929e-7f ? (s - b.min) / b.range : 1.0f;
        return std::min(std::max(v, 0.0f), 1.0f);
    };
    const Bounds fb = bounds(fast, n_fast), qb = bounds(quality, n_quality);
    struct Pair {
        std::string_view doc;
        float fast = 0.f, quality = 0.f;
        bool has_fast = false, has_quality = false;
        uint32_t index = 0;
    };
    std::unordered_map<std::string_view, size_t> slot;
    std::vector<Pair> merged;
    merged.reserve((size_t)std::max(n_fast, n_quality) * 13 / 10 + 1);
    for (uint32_t i = 0; i < n_fast; ++i) {
        auto it = slot.find(sv(fast[i]));
        if (it == slot.end()) {
            Pair p;
            p.doc = sv(fast[i]);
            p.index = fast[i].index;
            it = slot.emplace(p.doc, merged.size()).first;
            merged.push_back(p);
        }
        Pair& p = merged[it->second];
        if (!p.has_fast) {  // best-first input: keep the first (best) score and its index
            p.fast = apply(fb, fast[i].score);
            p.has_fast = true;
            p.index = fast[i].index;
        }
    }
    for (uint32_t i = 0; i < n_quality; ++i) {
        auto it = slot.find(sv(quality[i]));
        if (it == slot.end()) {
            Pair p;
            p.doc = sv(quality[i]);
            p.index = quality[i].index;
            it = slot.emplace(p.doc, merged.size()).first;
            merged.push_back(p);
        }
        Pair& p = merged[it->second];
        if (!p.has_quality) {
            p.quality = apply(qb, quality[i].score);
            p.has_quality = true;
        }
    }
    std::vector<fsgpu_scored_doc> blended(merged.size());
    for (size_t i = 0; i < merged.size(); ++i) {
        const Pair& p = merged[i];
        float score;
        if (p.has_fast && p.has_quality) score = std::fmaf(alpha, p.quality, (1.0f - alpha) * p.fast);
        else if (p.has_fast) score = p.fast;
        else if (p.has_quality) score = p.quality;
        else score = 0.0f;
        if (!std::isfinite(score)) score = 0.0f;
        blended[i] = fsgpu_scored_doc{p.doc.data(), (uint32_t)p.doc.size(), score, p.index};
    }
    std::sort(blended.begin(), blended.end(), [](const fsgpu_scored_doc& a, const fsgpu_scored_doc& b) {
        const int32_t x = total_key32(a.score), y = total_key32(b.score);
        if (x != y) return x > y;
        return std::string_view(a.doc_id, a.doc_id_len) < std::string_view(b.doc_id, b.doc_id_len);
    });
    std::copy(blended.begin(), blended.end(), out);
    *out_count = (uint32_t)blended.size();
    return FSGPU_OK;
}

// blend_two_tier_aligned (blend.rs:213-294): the same normalisation, merge and order as fsgpu_blend_two_tier with the quality tier
// given as per-position optional scores of the fast hits themselves.
extern "C" fsgpu_status fsgpu_blend_two_tier_aligned(const fsgpu_scored_doc* fast, uint32_t n_fast, const float* quality_scores,
                                                      const uint8_t* quality_present, float blend_factor, fsgpu_scored_doc* out,
                                                      uint32_t* out_count) {
    if (!out_count || (n_fast && (!fast || !out || !quality_scores || !quality_present))) return FSGPU_ERR_NULL_ARGUMENT;
    *out_count = 0;
    const float alpha = std::isfinite(blend_factor) ? std::min(std::max(blend_factor, 0.0f), 1.0f) : 0.7f;
    struct Bounds {
        float min = std::numeric_limits<float>::infinity(), max = -std::numeric_limits<float>::infinity(), range = 0.f;
        bool saw = false;
        void add(float v) {
            if (std::isfinite(v)) {
                min = std::min(min, v);
                max = std::max(max, v);
                saw = true;
            }
        }
        float apply(float s) const {
            if (!saw || !std::isfinite(s)) return 0.0f;
            const float v = range > 1.1920929e-7f ? (s - min) / range : 1.0f;
            return std::min(std::max(v, 0.0f), 1.0f);
        }
    } fb, qb;
    for (uint32_t i = 0; i < n_fast; ++i) {
        fb.add(fast[i].score);
        if (quality_present[i]) qb.add(quality_scores[i]);
    }
    fb.range = fb.max - fb.min;
    qb.range = qb.max - qb.min;
    struct Pair {
        std::string_view doc;
        float fast = 0.f, quality = 0.f;
        bool has_fast = false, has_quality = false;
        uint32_t index = 0;
    };
    std::unordered_map<std::string_view, size_t> slot;
    std::vector<Pair> merged;
    merged.reserve((size_t)n_fast * 13 / 10 + 1);
    for (uint32_t i = 0; i < n_fast; ++i) {
        auto it = slot.find(sv(fast[i]));
        if (it == slot.end()) {
            Pair p;
            p.doc = sv(fast[i]);
            p.index = fast[i].index;
            it = slot.emplace(p.doc, merged.size()).first;
            merged.push_back(p);
        }
        Pair& p = merged[it->second];
        if (!p.has_fast) {   // best-first input: the first (best) score and its index
            p.fast = fb.apply(fast[i].score);
            p.has_fast = true;
            p.index = fast[i].index;
        }
        if (quality_present[i] && !p.has_quality) {
            p.quality = qb.apply(quality_scores[i]);
            p.has_quality = true;
        }
    }
    std::vector<fsgpu_scored_doc> blended(merged.size());
    for (size_t i = 0; i < merged.size(); ++i) {
        const Pair& p = merged[i];
        float score = p.has_quality ? std::fmaf(alpha, p.quality, (1.0f - alpha) * p.fast) : p.fast;
        if (!std::isfinite(score)) score = 0.0f;
        blended[i] = fsgpu_scored_doc{p.doc.data(), (uint32_t)p.doc.size(), score, p.index};
    }
    std::sort(blended.begin(), blended.end(), [](const fsgpu_scored_doc& a, const fsgpu_scored_doc& b) {
        const int32_t x = total_key32(a.score), y = total_key32(b.score);
        if (x != y) return x > y;
        return std::string_view(a.doc_id, a.doc_id_len) < std::string_view(b.doc_id, b.doc_id_len);
    });
    std::copy(blended.begin(), blended.end(), out);
    *out_count = (uint32_t)blended.size();
    return FSGPU_OK;
}

// rerank_step_with_combine after the model call (crates/frankensearch-rerank/src/pipeline.rs:125-360): the scores of the
// candidates WITH text inside the window, in window order, land on their candidates (stale rerank scores in the window cleared,
// non-finite scores skipped), then the window is reordered — PureReorder: rerank score desc (non-finite as -inf, total order),
// doc_id asc (compare_by_rerank_score :290-303); RrfCombine: 1/(k + pre_rank) + 1/(k + rerank_rank) in f64 desc, doc_id asc
// (apply_rrf_combine :322-360).  Both sorts are stable, as Rust's sort_by is.  Candidates past the window keep their order.
extern "C" fsgpu_status fsgpu_rerank_apply(fsgpu_rerank_candidate* candidates, uint32_t n, const uint8_t* has_text, const float* scores,
                                           uint32_t n_scores, uint32_t top_k_rerank, uint32_t min_candidates, int32_t combine, float k,
                                           uint8_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (combine != FSGPU_RERANK_PURE_REORDER && combine != FSGPU_RERANK_RRF_COMBINE) return FSGPU_ERR_INVALID_CONFIG;
    if (n > 0 && !candidates) return FSGPU_ERR_NULL_ARGUMENT;
    if (n < min_candidates) return FSGPU_OK;   // too few candidates (:135-142)
    const uint32_t window = std::min(n, top_k_rerank);
    std::vector<uint32_t> included;   // window positions of the candidates with text, in order
    for (uint32_t i = 0; i < window; ++i)
        if (!has_text || has_text[i]) included.push_back(i);
    if (included.size() < min_candidates) return FSGPU_OK;   // too few with text (:165-172)
    if (n_scores != included.size()) return FSGPU_OK;        // score count mismatch: skipped (:205-213)
    if (n_scores > 0 && !scores) return FSGPU_ERR_NULL_ARGUMENT;
    const float none = std::numeric_limits<float>::quiet_NaN();
    for (uint32_t i = 0; i < window; ++i) candidates[i].rerank_score = none;   // clear_rerank_scores (:265-270)
    for (uint32_t j = 0; j < n_scores; ++j)
        if (std::isfinite(scores[j])) candidates[included[j]].rerank_score = scores[j];
    auto doc = [](const fsgpu_rerank_candidate& c) { return std::string_view(c.doc_id, c.doc_id_len); };
    auto sort_key = [](const fsgpu_rerank_candidate& c) {
        return total_key32(std::isfinite(c.rerank_score) ? c.rerank_score : -std::numeric_limits<float>::infinity());
    };
    auto by_rerank = [&](const fsgpu_rerank_candidate& a, const fsgpu_rerank_candidate& b) {
        const int32_t ka = sort_key(a), kb = sort_key(b);
        if (ka != kb) return ka > kb;
        return doc(a) < doc(b);
    };
    if (combine == FSGPU_RERANK_PURE_REORDER) {
        std::stable_sort(candidates, candidates + window, by_rerank);
    } else if (window >= 2) {
        const double kf = (double)(std::isnan(k) ? 1.0f : std::max(k, 1.0f));   // f32::max: a NaN k gives 1
        std::vector<uint32_t> order(window);
        for (uint32_t i = 0; i < window; ++i) order[i] = i;
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return by_rerank(candidates[a], candidates[b]); });
        std::vector<double> key(window);
        for (uint32_t r = 0; r < window; ++r) key[order[r]] = 1.0 / (kf + (double)order[r]) + 1.0 / (kf + (double)r);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
            const int64_t ka = total_key64(key[a]), kb = total_key64(key[b]);
            if (ka != kb) return ka > kb;
            return doc(candidates[a]) < doc(candidates[b]);
        });
        std::vector<fsgpu_rerank_candidate> snap(candidates, candidates + window);
        for (uint32_t i = 0; i < window; ++i) candidates[i] = snap[order[i]];
    }
    if (out_applied) *out_applied = 1;
    return FSGPU_OK;
}

// ---- Maximum Marginal Relevance: mmr_rerank (crates/frankensearch-fusion/src/mmr.rs:103-319), every value in f64 ----
// (this file is built with -ffp-contract=off: `acc += a * b` stays a multiply and an add, as rustc emits it; the products are exact
// in f64 either way, the ORDER of the additions is what the bits depend on)
namespace fsgpu {

namespace {
constexpr double kF64Epsilon = std::numeric_limits<double>::epsilon();

// cosine_sim (mmr.rs:254-279): the ragged-pool form, one accumulator each for the dot and both norms over the shorter length
double mmr_cosine_sim(const float* a, uint32_t la, const float* b, uint32_t lb) {
    const uint32_t len = std::min(la, lb);
    if (len == 0) return 0.0;
    double dot = 0.0, norm_a = 0.0, norm_b = 0.0;
    for (uint32_t i = 0; i < len; ++i) {
        const double ai = (double)a[i], bi = (double)b[i];
        dot += ai * bi;
        norm_a += ai * ai;
        norm_b += bi * bi;
    }
    const double denom = std::sqrt(norm_a) * std::sqrt(norm_b);
    if (denom < kF64Epsilon) return 0.0;
    return dot / denom;
}

// cosine_sim_pre (mmr.rs:285-319): four accumulators, element i to acc[i % 4], ((a0 + a1) + a2) + a3, the tail in order
double mmr_cosine_sim_pre(const float* a, const float* b, uint32_t len, double root_a, double root_b) {
    if (len == 0) return 0.0;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    const uint32_t chunks = len / 4;
    for (uint32_t c = 0; c < chunks; ++c) {
        const uint32_t i = c * 4;
        acc[0] += (double)a[i] * (double)b[i];
        acc[1] += (double)a[i + 1] * (double)b[i + 1];
        acc[2] += (double)a[i + 2] * (double)b[i + 2];
        acc[3] += (double)a[i + 3] * (double)b[i + 3];
    }
    double dot = ((acc[0] + acc[1]) + acc[2]) + acc[3];
    for (uint32_t i = chunks * 4; i < len; ++i) dot += (double)a[i] * (double)b[i];
    const double denom = root_a * root_b;
    if (denom < kF64Epsilon) return 0.0;
    return dot / denom;
}
}  // namespace

double mmr_clamped_lambda(double lambda) {
    if (!std::isfinite(lambda) || lambda < 0.0) return 0.0;
    return lambda > 1.0 ? 1.0 : lambda;
}

void mmr_rerank_host(const double* scores, const float* const* vectors, const uint32_t* lengths, uint32_t len, uint32_t k, double lambda_in,
                     uint32_t candidate_pool, uint32_t* out_order, uint32_t* out_count, double* out_sims) {
    *out_count = 0;
    const uint32_t n = std::min(len, candidate_pool);
    if (n == 0 || k == 0) return;
    k = std::min(k, n);
    const double lambda = mmr_clamped_lambda(lambda_in), diversity_weight = 1.0 - lambda;
    double min_score = std::numeric_limits<double>::infinity(), max_score = -std::numeric_limits<double>::infinity();
    for (uint32_t i = 0; i < n; ++i)
        if (std::isfinite(scores[i])) {
            min_score = scores[i] < min_score ? scores[i] : min_score;
            max_score = scores[i] > max_score ? scores[i] : max_score;
        }
    const double score_range = max_score - min_score;
    std::vector<double> norm_scores(n);
    for (uint32_t i = 0; i < n; ++i)
        norm_scores[i] = !std::isfinite(scores[i]) ? 0.0 : score_range < kF64Epsilon ? 1.0 : (scores[i] - min_score) / score_range;
    bool uniform = true;
    for (uint32_t i = 0; i < n; ++i) uniform = uniform && lengths[i] == lengths[0];
    std::vector<double> root(uniform ? n : 0);
    for (uint32_t i = 0; uniform && i < n; ++i) {
        double norm = 0.0;
        for (uint32_t e = 0; e < lengths[i]; ++e) {
            const double x = (double)vectors[i][e];
            norm += x * x;
        }
        root[i] = std::sqrt(norm);
    }
    auto sim = [&](uint32_t i, uint32_t j) {
        return uniform ? mmr_cosine_sim_pre(vectors[i], vectors[j], lengths[0], root[i], root[j])
                       : mmr_cosine_sim(vectors[i], lengths[i], vectors[j], lengths[j]);
    };
    if (out_sims)
        for (uint32_t i = 0; i < n; ++i)
            for (uint32_t j = 0; j < n; ++j) out_sims[(size_t)i * n + j] = sim(i, j);
    uint32_t first = 0;
    double best_s = -std::numeric_limits<double>::infinity();
    for (uint32_t i = 0; i < n; ++i)
        if (norm_scores[i] > best_s) first = i, best_s = norm_scores[i];
    std::vector<uint8_t> remaining(n, 1);
    uint32_t count = 0;
    out_order[count++] = first;
    remaining[first] = 0;
    std::vector<double> max_sim(n, -std::numeric_limits<double>::infinity());
    for (uint32_t i = 0; i < n; ++i)
        if (remaining[i]) max_sim[i] = sim(i, first);
    for (uint32_t round = 1; round < k; ++round) {
        uint32_t best_idx = 0xffffffffu;
        double best_mmr = -std::numeric_limits<double>::infinity();
        for (uint32_t i = 0; i < n; ++i) {
            if (!remaining[i]) continue;
            const double mmr = std::fma(lambda, norm_scores[i], -(diversity_weight * max_sim[i]));
            if (mmr > best_mmr) best_mmr = mmr, best_idx = i;
        }
        if (best_idx == 0xffffffffu) break;
        out_order[count++] = best_idx;
        remaining[best_idx] = 0;
        for (uint32_t i = 0; i < n; ++i)
            if (remaining[i]) {
                const double s = sim(i, best_idx);
                if (s > max_sim[i]) max_sim[i] = s;
            }
    }
    *out_count = count;
}

}  // namespace fsgpu

extern "C" fsgpu_status fsgpu_mmr_config_default(fsgpu_mmr_config* config) {
    if (!config) return FSGPU_ERR_NULL_ARGUMENT;
    std::memset(config, 0, sizeof(*config));
    config->lambda = 0.7;
    config->candidate_pool = 30;
    return FSGPU_OK;
}

extern "C" fsgpu_status fsgpu_mmr_rerank(const double* scores, const float* const* vectors, const uint32_t* lengths, uint32_t n, uint32_t k,
                                         double lambda, uint32_t candidate_pool, uint32_t* out_order, uint32_t* out_count, double* out_sims) {
    if (!out_count) return FSGPU_ERR_NULL_ARGUMENT;
    *out_count = 0;
    if (n && (!scores || !vectors || !lengths || !out_order)) return FSGPU_ERR_NULL_ARGUMENT;
    const uint32_t pool = std::min(n, candidate_pool);
    for (uint32_t i = 0; i < pool; ++i)
        if (lengths[i] && !vectors[i]) return FSGPU_ERR_NULL_ARGUMENT;
    try {
        fsgpu::mmr_rerank_host(scores, vectors, lengths, n, k, lambda, candidate_pool, out_order, out_count, out_sims);
    } catch (...) {
        return FSGPU_ERR_DEVICE;   // host allocation failed
    }
    return FSGPU_OK;
}

// ---- query hubness: compute_query_hubness / apply_hubness_penalty (crates/frankensearch-fusion/src/hubness.rs) ----
// (this file is built with -ffp-contract=off: every `acc + a * b` below is a multiply and an add, as in simd.rs:134-222)
namespace fsgpu {

float hubness_dot(const float* a, const float* b, size_t n, int hreduce) {
    const size_t groups = n / 32, chunks = n / 8;
    float acc[4][8] = {};
    for (size_t g = 0; g < groups; ++g)   // simd.rs:160-190: accumulator x takes elements [32 g + 8 x, 32 g + 8 x + 8)
        for (int x = 0; x < 4; ++x)
            for (int j = 0; j < 8; ++j) {
                const size_t o = g * 32 + (size_t)x * 8 + (size_t)j;
                const float p = a[o] * b[o];
                acc[x][j] = acc[x][j] + p;
            }
    float v[8];
    for (int j = 0; j < 8; ++j) v[j] = (acc[0][j] + acc[1][j]) + (acc[2][j] + acc[3][j]);
    for (size_t c = groups * 4; c < chunks; ++c)   // leftover chunks join AFTER the tree (the f16 byte dot adds them to s0 before it)
        for (int j = 0; j < 8; ++j) {
            const float p = a[c * 8 + (size_t)j] * b[c * 8 + (size_t)j];
            v[j] = v[j] + p;
        }
    float result;
    if (hreduce == FSGPU_HREDUCE_SEQ) {
        const float lo = ((v[0] + v[1]) + v[2]) + v[3];
        const float hi = ((v[4] + v[5]) + v[6]) + v[7];
        result = lo + hi;
    } else if (hreduce == FSGPU_HREDUCE_AVX) {
        const float s0 = v[0] + v[4], s1 = v[1] + v[5], s2 = v[2] + v[6], s3 = v[3] + v[7];
        const float lo = s0 + s2, hi = s1 + s3;
        result = lo + hi;
    } else {
        const float lo = (v[0] + v[2]) + (v[1] + v[3]);
        const float hi = (v[4] + v[6]) + (v[5] + v[7]);
        result = lo + hi;
    }
    for (size_t i = chunks * 8; i < n; ++i) {   // the tail is a multiply and an add too (the byte dots fuse theirs)
        const float p = a[i] * b[i];
        result = result + p;
    }
    return result;
}

float hubness_mean(const uint32_t* keys_desc, uint32_t k) {
    if (k == 1) return hubness_value(keys_desc[0]) / 1.0f;
    float s = hubness_value(keys_desc[0]);
    for (uint32_t i = 1; i + 1 < k; ++i) s = s + hubness_value(keys_desc[i]);
    return (hubness_value(keys_desc[k - 1]) + s) / (float)k;   // `*pivot + top.iter().sum()`, `/ k as f32` (hubness.rs:136-137)
}

namespace {
uint32_t hubness_threads(uint32_t asked) {
    if (asked) return std::min(asked, 64u);
    uint32_t n = 16;
    if (const char* env = std::getenv("OMP_NUM_THREADS")) {
        const long v = std::strtol(env, nullptr, 10);
        if (v >= 1) n = (uint32_t)std::min(v, 16l);
    }
    return n;
}
}  // namespace

void query_hubness_host(const float* const* docs, const uint32_t* doc_lens, uint64_t n_docs, const float* const* queries,
                        const uint32_t* query_lens, uint32_t n_queries, uint32_t kq, int hreduce, float* out, float* out_topk,
                        uint32_t threads) {
    if (n_queries == 0 || kq == 0) {   // hubness.rs:110-112
        for (uint64_t d = 0; d < n_docs; ++d) out[d] = 0.0f;
        return;
    }
    const uint32_t k = std::min(kq, n_queries);
    std::atomic<bool> failed{false};
    auto range = [&](uint64_t lo, uint64_t hi) {
        try {   // (a worker's allocation failure must reach the caller as a status, not std::terminate)
            std::vector<uint32_t> keys(n_queries);
            for (uint64_t d = lo; d < hi; ++d) {
                for (uint32_t j = 0; j < n_queries; ++j)
                    keys[j] = hubness_key(hubness_dot(docs[d], queries[j], std::min(doc_lens[d], query_lens[j]), hreduce));
                std::partial_sort(keys.begin(), keys.begin() + k, keys.end(), std::greater<uint32_t>());
                out[d] = hubness_mean(keys.data(), k);
                if (out_topk)
                    for (uint32_t i = 0; i < k; ++i) out_topk[d * k + i] = hubness_value(keys[i]);
            }
        } catch (...) {
            failed.store(true);
        }
    };
    // rows are independent (hubness.rs:96-102): contiguous row ranges, one per thread
    const uint64_t work = n_docs * (uint64_t)n_queries;
    const uint32_t nt = work < 10000 ? 1u : (uint32_t)std::min<uint64_t>(hubness_threads(threads), n_docs);
    std::vector<std::thread> pool;
    uint32_t started = 0;
    if (nt > 1) {
        try {
            pool.reserve(nt);
            for (; started < nt; ++started) pool.emplace_back(range, n_docs * started / nt, n_docs * (started + 1) / nt);
        } catch (...) {   // no more threads to be had: the calling thread takes the ranges that are left
        }
    }
    if (started < nt) range(n_docs * started / nt, n_docs);
    for (std::thread& th : pool) th.join();
    if (failed.load()) throw std::bad_alloc();
}

}  // namespace fsgpu

extern "C" fsgpu_status fsgpu_hubness_config_default(fsgpu_hubness_config* config) {
    if (!config) return FSGPU_ERR_NULL_ARGUMENT;
    std::memset(config, 0, sizeof(*config));
    config->beta = 0.2f;   // HubnessConfig::default (hubness.rs:46-50)
    config->kq = 10;
    return FSGPU_OK;
}

extern "C" fsgpu_status fsgpu_query_hubness(const float* const* docs, const uint32_t* doc_lens, uint64_t n_docs, const float* const* queries,
                                            const uint32_t* query_lens, uint32_t n_queries, uint32_t kq, int32_t hreduce, float* out) {
    if (n_docs && (!out || !docs || !doc_lens)) return FSGPU_ERR_NULL_ARGUMENT;
    if (n_queries && (!queries || !query_lens)) return FSGPU_ERR_NULL_ARGUMENT;
    if (hreduce < FSGPU_HREDUCE_SSE2 || hreduce > FSGPU_HREDUCE_SEQ) return FSGPU_ERR_INVALID_CONFIG;
    for (uint64_t d = 0; d < n_docs; ++d)
        if (doc_lens[d] && !docs[d]) return FSGPU_ERR_NULL_ARGUMENT;
    for (uint32_t j = 0; j < n_queries; ++j)
        if (query_lens[j] && !queries[j]) return FSGPU_ERR_NULL_ARGUMENT;
    try {
        fsgpu::query_hubness_host(docs, doc_lens, n_docs, queries, query_lens, n_queries, kq, hreduce, out, nullptr);
    } catch (...) {
        return FSGPU_ERR_DEVICE;   // host allocation failed (the ABI's status for a resource failure; fsgpu_mmr_rerank does the same)
    }
    return FSGPU_OK;
}

// apply_hubness_penalty (hubness.rs:67-86) in place, then — resort != 0 — correct_phase1_pool's sort by VectorHit::cmp_rank
// (searcher.rs:769-777, types.rs:101-133): score descending with NaN as -inf under total_cmp, doc_id bytes ascending; stable.
extern "C" fsgpu_status fsgpu_apply_hubness_penalty(fsgpu_scored_doc* hits, uint32_t n, const float* table, uint64_t table_len,
                                                    const fsgpu_hubness_config* config, int32_t resort, uint8_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (n && !hits) return FSGPU_ERR_NULL_ARGUMENT;
    if (table_len && !table) return FSGPU_ERR_NULL_ARGUMENT;
    fsgpu_hubness_config cfg;
    fsgpu_hubness_config_default(&cfg);
    if (config) {
        for (uint32_t r : config->reserved)
            if (r != 0) return FSGPU_ERR_INVALID_CONFIG;
        cfg = *config;
    }
    if (!std::isfinite(cfg.beta) || cfg.beta <= 0.0f) return FSGPU_OK;   // HubnessConfig::is_identity
    for (uint32_t i = 0; i < n; ++i) {
        const float r = hits[i].index < table_len ? table[hits[i].index] : 0.0f;
        const float p = cfg.beta * r;
        hits[i].score = hits[i].score - p;
    }
    if (resort)
        std::stable_sort(hits, hits + n, [](const fsgpu_scored_doc& a, const fsgpu_scored_doc& b) {
            const float inf = std::numeric_limits<float>::infinity();
            const int32_t x = total_key32(std::isnan(a.score) ? -inf : a.score), y = total_key32(std::isnan(b.score) ? -inf : b.score);
            if (x != y) return x > y;
            return sv(a) < sv(b);
        });
    if (out_applied) *out_applied = 1;
    return FSGPU_OK;
}

// ---- k-NN graph diffusion: neighbor_smooth / neighbor_smooth_ranked (crates/frankensearch-fusion/src/smooth.rs:84-153, 176-276) ----
// The reference keys the pool and the graph by doc-id string; here both are keyed by ROW (hits[i].index, the table of
// fsgpu_index_build_knn_graph): include/fsgpu.h states the deviation.

extern "C" fsgpu_status fsgpu_smooth_config_default(fsgpu_smooth_config* config) {
    if (!config) return FSGPU_ERR_NULL_ARGUMENT;
    std::memset(config, 0, sizeof(*config));
    config->alpha = 0.3f;   // SmoothConfig::default (smooth.rs:53-61)
    config->m = 10;
    config->mutual = 0;
    return FSGPU_OK;
}

extern "C" fsgpu_status fsgpu_neighbor_smooth(fsgpu_scored_doc* hits, uint32_t n, const uint32_t* graph_rows, uint64_t graph_len,
                                              uint32_t graph_width, const fsgpu_smooth_config* config, int32_t resort, uint8_t* out_applied) {
    if (out_applied) *out_applied = 0;
    if (n && !hits) return FSGPU_ERR_NULL_ARGUMENT;
    fsgpu_smooth_config cfg;
    fsgpu_smooth_config_default(&cfg);
    if (config) {
        for (uint32_t r : config->reserved)
            if (r != 0) return FSGPU_ERR_INVALID_CONFIG;
        cfg = *config;
    }
    // SmoothConfig::is_identity, an empty graph, an empty pool (smooth.rs:66-68, 89-91, 270-272): nothing is touched, nothing is sorted
    if (!std::isfinite(cfg.alpha) || cfg.alpha <= 0.0f || cfg.m == 0) return FSGPU_OK;
    if (!graph_rows || graph_len == 0 || graph_width == 0 || n == 0) return FSGPU_OK;
    try {
        // row -> score; a row that occurs twice counts with its last occurrence (the AHashMap insert of smooth.rs:101, 186-189)
        std::unordered_map<uint32_t, float> pool;
        pool.reserve((size_t)n * 2);
        for (uint32_t i = 0; i < n; ++i) pool[hits[i].index] = hits[i].score;
        const uint32_t walk = std::min(cfg.m, graph_width);
        const float alpha = cfg.alpha, keep = 1.0f - alpha;
        std::vector<float> smoothed(n);
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t row = hits[i].index;
            float sum = 0.0f;
            uint32_t count = 0;
            if (row < graph_len) {   // (beyond the table: a WAL virtual row or 0xffffffff — no edges, nobody's neighbour)
                const uint32_t* list = graph_rows + (uint64_t)row * graph_width;
                for (uint32_t e = 0; e < walk; ++e) {   // every walked entry counts as examined, in the pool or not
                    const uint32_t nb = list[e];
                    if (nb == 0xffffffffu) break;
                    const auto it = pool.find(nb);
                    if (it == pool.end()) continue;
                    if (cfg.mutual) {   // reciprocity over the neighbour's WHOLE stored list (the reference's set is uncapped)
                        if (nb >= graph_len) continue;
                        const uint32_t* back = graph_rows + (uint64_t)nb * graph_width;
                        bool mutual = false;
                        for (uint32_t x = 0; x < graph_width && !mutual; ++x) mutual = back[x] == row;
                        if (!mutual) continue;
                    }
                    sum = sum + it->second;
                    ++count;
                }
            }
            const float mean = count == 0 ? hits[i].score : sum / (float)count;
            const float a = keep * hits[i].score, b = alpha * mean;
            smoothed[i] = a + b;
        }
        for (uint32_t i = 0; i < n; ++i) hits[i].score = smoothed[i];
        if (resort)   // VectorHit::cmp_rank, as fsgpu_apply_hubness_penalty sorts
            std::stable_sort(hits, hits + n, [](const fsgpu_scored_doc& a, const fsgpu_scored_doc& b) {
                const float inf = std::numeric_limits<float>::infinity();
                const int32_t x = total_key32(std::isnan(a.score) ? -inf : a.score), y = total_key32(std::isnan(b.score) ? -inf : b.score);
                if (x != y) return x > y;
                return sv(a) < sv(b);
            });
    } catch (...) {
        return FSGPU_ERR_DEVICE;   // host allocation failed (the ABI's status for a resource failure)
    }
    if (out_applied) *out_applied = 1;
    return FSGPU_OK;
}

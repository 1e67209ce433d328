// ann_index.cpp — the host side of the graph ANN search (ann_index.hpp; include/fsgpu.h, "graph ANN search").
//
// A search is ONE launch of ann_search_kernel (a workgroup per query) on the index's stream, one copy of the counts, the two
// per-query counters and (host form) the hits back, and — for the queries the beam left short of min(k, live rows) — the index's own exact batched search
// (hnsw.rs:1150-1190).  certify_ef is certify_ef_search (hnsw.rs:1354-1386): the exact answers once, the beam per candidate ef in
// ascending order, the conformal bound after each, and no launch past the first ef that meets the target.
#include "ann_index.hpp"

#include <algorithm>
#include <cmath>

#include "vector_index_internal.hpp"

namespace fsgpu {

using detail::make_error;
using detail::ok;

// ---- the recall certificates (recall_certificate.rs) ----------------------------------------------------------------------------

namespace {

double clamp01(double v) { return v < 0.0 ? 0.0 : (v > 1.0 ? 1.0 : v); }   // (a NaN stays a NaN, as f64::clamp)
bool level_ok(double v) { return v >= 0.0 && v < 1.0; }                    // (0.0..1.0).contains: false for a NaN

std::vector<double> finite_of(const double* recalls, uint64_t n) {
    std::vector<double> out;
    out.reserve((size_t)n);
    for (uint64_t i = 0; i < n; ++i)
        if (std::isfinite(recalls[i])) out.push_back(recalls[i]);
    return out;
}

}  // namespace

double conformal_recall_lower_bound(const double* recalls, uint64_t n, double alpha) {
    if (!level_ok(alpha)) return 0.0;
    std::vector<double> sorted = finite_of(recalls, n);
    const size_t m = sorted.size();
    if (m == 0) return 0.0;
    const size_t rank = (size_t)std::floor(alpha * ((double)m + 1.0));
    if (rank == 0) return 0.0;
    std::sort(sorted.begin(), sorted.end());
    return clamp01(sorted[std::min(rank - 1, m - 1)]);
}

double mean_recall_lower_bound(const double* recalls, uint64_t n, double delta) {
    if (!level_ok(delta)) return 0.0;
    const std::vector<double> finite = finite_of(recalls, n);
    if (finite.empty()) return 0.0;
    const double nf = (double)finite.size();
    double sum = 0.0;
    for (double v : finite) sum += v;
    const double mean = sum / nf;
    const double radius = std::sqrt(std::log(1.0 / delta) / (2.0 * nf));
    return clamp01(mean - radius);
}

double mean_recall_lower_bound_bernstein(const double* recalls, uint64_t n, double delta) {
    if (!level_ok(delta)) return 0.0;
    const std::vector<double> finite = finite_of(recalls, n);
    if (finite.size() < 2) return 0.0;
    const double nf = (double)finite.size();
    double sum = 0.0;
    for (double v : finite) sum += v;
    const double mean = sum / nf;
    double sq = 0.0;
    for (double v : finite) sq += (v - mean) * (v - mean);
    const double var = sq / (nf - 1.0);
    const double ln = std::log(2.0 / delta);
    return clamp01(mean - std::sqrt(2.0 * var * ln / nf) - 7.0 * ln / (3.0 * (nf - 1.0)));
}

bool certified_min_ef(const uint32_t* efs, const double* const* recalls, const uint64_t* lens, uint32_t n, double target, double level,
                      bool mean_bound, CertifiedEf* out) {
    if (n == 0) return false;
    std::vector<uint32_t> order(n);
    for (uint32_t i = 0; i < n; ++i) order[i] = i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return efs[x] < efs[y]; });
    bool have = false;
    CertifiedEf best;
    for (uint32_t i : order) {
        const double bound = mean_bound ? mean_recall_lower_bound_bernstein(recalls[i], lens[i], level)
                                        : conformal_recall_lower_bound(recalls[i], lens[i], level);
        CertifiedEf c;
        c.ef_search = efs[i];
        c.certified_recall = bound;
        c.meets_target = bound >= target;
        if (c.meets_target) {
            *out = c;
            return true;
        }
        if (!have || bound > best.certified_recall) {
            best = c;
            have = true;
        }
    }
    *out = best;
    return true;
}

double recall_at_k_of_rows(const uint32_t* approx, uint32_t n_approx, const uint32_t* exact, uint32_t n_exact) {
    if (n_exact == 0) return 1.0;
    uint32_t overlap = 0;
    for (uint32_t i = 0; i < n_exact; ++i)
        if (std::find(approx, approx + n_approx, exact[i]) != approx + n_approx) ++overlap;
    return (double)overlap / (double)n_exact;
}

// ---- the launch --------------------------------------------------------------------------------------------------------------------

SearchError VectorIndex::ann_launch(AnnSearchArgs a, uint32_t nq, hipStream_t stream) {
    if (catalog_only_ || !slab_dev_) return make_error(FSGPU_ERR_INVALID_CONFIG, "this index holds no slab of its own");
    a.slab = slab_dev_;
    a.live = reinterpret_cast<const u64*>(live_dev_);
    a.nrows = (uint32_t)nrows_;
    a.dim = dim_;
    a.row_base = (uint32_t)row_base_;
    a.row_stride = row_stride_ ? row_stride_ : dim_ * (f32_ ? 4u : 2u);
    a.slab_f32 = f32_ ? 1u : 0u;
    a.hreduce = hreduce;
    if (!ann_args_ok(a)) return make_error(FSGPU_ERR_INVALID_CONFIG, "the ANN search's limits do not hold for this call");
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_HIP(launch_ann_search(a, nq, stream));
    return ok();
}

// ---- the handle --------------------------------------------------------------------------------------------------------------------

AnnIndex::~AnnIndex() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    if (ev_begin_) (void)hipEventDestroy(ev_begin_);
    if (ev_end_) (void)hipEventDestroy(ev_end_);
    if (pin_) (void)hipHostFree(pin_);
    graph_.release();
    ws_.release();
}

SearchError AnnIndex::init(VectorIndex* index, const uint32_t* graph_rows, uint64_t graph_len, uint32_t graph_width, const AnnConfig& config) {
    const uint64_t n = index->record_count();
    if (graph_len != n)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the table has " + std::to_string(graph_len) + " lists, the index " + std::to_string(n) + " rows");
    if (graph_width < 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "the table's width must be at least 1");
    if (n >= 0xffffffffull) return make_error(FSGPU_ERR_INVALID_CONFIG, "row ids must fit 32 bits");
    if (index->dimension() > kAnnMaxDim)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the ANN search keeps the query in LDS: at most " + std::to_string(kAnnMaxDim) + " dimensions");
    AnnConfig c = config;
    if (c.degree == 0) c.degree = graph_width;
    if (c.degree > graph_width) return make_error(FSGPU_ERR_INVALID_CONFIG, "degree exceeds the table's width");
    if (c.expand < 1 || c.expand > kAnnMaxExpand) return make_error(FSGPU_ERR_INVALID_CONFIG, "expand must be 1 .. 8");
    if (c.max_iters < 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "max_iters must be at least 1");
    if ((uint64_t)c.expand * c.degree > kAnnMaxStepRows)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "expand * degree exceeds " + std::to_string(kAnnMaxStepRows) + ", the rows of one step");
    if ((uint64_t)c.max_iters * c.expand * c.degree > kAnnMaxAdmitted)
        return make_error(FSGPU_ERR_INVALID_CONFIG,
                          "max_iters * expand * degree exceeds " + std::to_string(kAnnMaxAdmitted) + ", what the visited table in LDS holds");
    if (c.n_entry < 1) return make_error(FSGPU_ERR_INVALID_CONFIG, "n_entry must be at least 1");
    if (c.n_entry > n) c.n_entry = (uint32_t)n;
    if (c.n_entry > kAnnMaxEntry) return make_error(FSGPU_ERR_INVALID_CONFIG, "n_entry exceeds " + std::to_string(kAnnMaxEntry));
    if (index->device() < 0) return make_error(FSGPU_ERR_NO_DEVICE, "index has no device");
    device_ = index->device();
    FSGPU_HIP(hipSetDevice(device_));
    const size_t bytes = (size_t)n * graph_width * 4;
    FSGPU_TRY(graph_.reserve(std::max<size_t>(bytes, 4)));
    if (bytes) FSGPU_HIP(hipMemcpy(graph_.ptr, graph_rows, bytes, hipMemcpyHostToDevice));
    FSGPU_HIP(hipEventCreate(&ev_begin_));
    FSGPU_HIP(hipEventCreate(&ev_end_));
    index_ = index;
    nrows_ = n;
    generation_ = index->generation();
    width_ = graph_width;
    cfg_ = c;
    return ok();
}

SearchError AnnIndex::check_call(uint32_t k, uint32_t ef) const {
    if (!index_) return make_error(FSGPU_ERR_INVALID_CONFIG, "the handle was not initialised");
    if (index_->generation() != generation_ || index_->record_count() != nrows_)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "the table was made before the index was compacted or vacuumed: its row ids are stale");
    if (k < 1 || k > ef || ef > kAnnMaxEf)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "1 <= k <= ef <= 256 does not hold (k " + std::to_string(k) + ", ef " + std::to_string(ef) + ")");
    return ok();
}

SearchError AnnIndex::search(const float* queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t ef, uint32_t* out_rows,
                             float* out_scores, uint32_t* out_counts, uint32_t* out_flags, bool on_device, AnnStats* stats) {
    FSGPU_TRY(check_call(k, ef));
    const uint32_t dim = index_->dimension();
    if (query_len != dim)
        return make_error(FSGPU_ERR_DIMENSION_MISMATCH, "expected " + std::to_string(dim) + ", found " + std::to_string(query_len));
    AnnStats st;
    st.index_size = nrows_;
    st.dimension = dim;
    st.ef_search = ef;
    st.k_requested = k;
    st.queries = nq;
    auto done = [&]() {
        last_ = st;
        if (stats) *stats = st;
        return ok();
    };
    if (nq == 0) return done();
    FSGPU_HIP(hipSetDevice(index_->device()));
    hipStream_t stream = index_->stream();
    if (nrows_ == 0) {   // nothing indexed: count 0, flag 0 (min(k, live rows) = 0)
        if (on_device) {
            FSGPU_HIP(hipMemsetAsync(out_counts, 0, (size_t)nq * 4, stream));
            if (out_flags) FSGPU_HIP(hipMemsetAsync(out_flags, 0, (size_t)nq * 4, stream));
            FSGPU_HIP(hipStreamSynchronize(stream));
        } else {
            std::fill(out_counts, out_counts + nq, 0u);
            if (out_flags) std::fill(out_flags, out_flags + nq, 0u);
        }
        st.approximate = nq;
        return done();
    }

    // device block: counts | scored | steps (| rows | scores | queries for the host form); what comes back is its head, in ONE copy
    // into the handle's pinned block (five copies into pageable vectors are five staged transfers: a third of a lone query's time)
    auto align256 = [](size_t v) { return (v + 255) / 256 * 256; };
    const size_t hits = (size_t)nq * k * 4;
    const size_t o_scored = align256((size_t)nq * 4), o_steps = align256(o_scored + (size_t)nq * 4), o_rows = align256(o_steps + (size_t)nq * 4),
                 o_scores = align256(o_rows + (on_device ? 0 : hits)), o_q = align256(o_scores + (on_device ? 0 : hits)),
                 total = align256(o_q + (on_device ? 0 : (size_t)nq * dim * 4));
    FSGPU_TRY(ws_.reserve(total));
    if (pin_bytes_ < o_q) {
        if (pin_) (void)hipHostFree(pin_);
        pin_ = nullptr;
        pin_bytes_ = 0;
        FSGPU_HIP(hipHostMalloc(&pin_, o_q, hipHostMallocDefault));
        pin_bytes_ = o_q;
    }
    unsigned char* base = static_cast<unsigned char*>(ws_.ptr);
    unsigned char* pin = static_cast<unsigned char*>(pin_);
    if (!on_device) FSGPU_HIP(hipMemcpyAsync(base + o_q, queries, (size_t)nq * dim * 4, hipMemcpyHostToDevice, stream));
    AnnSearchArgs a{};
    a.graph = static_cast<const uint32_t*>(graph_.ptr);
    a.queries = on_device ? queries : reinterpret_cast<const float*>(base + o_q);
    a.width = width_;
    a.degree = cfg_.degree;
    a.expand = cfg_.expand;
    a.max_iters = cfg_.max_iters;
    a.n_entry = cfg_.n_entry;
    a.k = k;
    a.ef = ef;
    a.out_rows = on_device ? out_rows : reinterpret_cast<uint32_t*>(base + o_rows);
    a.out_scores = on_device ? out_scores : reinterpret_cast<float*>(base + o_scores);
    a.out_counts = on_device ? out_counts : reinterpret_cast<uint32_t*>(base);
    a.out_scored = reinterpret_cast<uint32_t*>(base + o_scored);
    a.out_steps = reinterpret_cast<uint32_t*>(base + o_steps);
    FSGPU_HIP(hipEventRecord(ev_begin_, stream));
    FSGPU_TRY(index_->ann_launch(a, nq, stream));
    FSGPU_HIP(hipEventRecord(ev_end_, stream));
    if (on_device) {
        FSGPU_HIP(hipMemcpyAsync(pin, out_counts, (size_t)nq * 4, hipMemcpyDeviceToHost, stream));
        FSGPU_HIP(hipMemcpyAsync(pin + o_scored, base + o_scored, o_rows - o_scored, hipMemcpyDeviceToHost, stream));
    } else {
        FSGPU_HIP(hipMemcpyAsync(pin, base, o_q, hipMemcpyDeviceToHost, stream));
    }
    FSGPU_HIP(hipStreamSynchronize(stream));
    const uint32_t* scored = reinterpret_cast<const uint32_t*>(pin + o_scored);
    const uint32_t* steps = reinterpret_cast<const uint32_t*>(pin + o_steps);
    std::vector<uint32_t> counts(reinterpret_cast<const uint32_t*>(pin), reinterpret_cast<const uint32_t*>(pin) + nq), flags(nq, 0u);
    uint32_t* rows = reinterpret_cast<uint32_t*>(pin + o_rows);   // (host form)
    float* scores = reinterpret_cast<float*>(pin + o_scores);
    float ms = 0.0f;
    FSGPU_HIP(hipEventElapsedTime(&ms, ev_begin_, ev_end_));
    st.device_ms = ms;
    st.launches = 1;
    for (uint32_t q = 0; q < nq; ++q) {
        st.rows_scored += scored[q];
        st.steps += steps[q];
    }

    // the fallback (hnsw.rs:1150-1190): count < min(k, live rows) -> the exact search answers
    std::vector<uint32_t> under;
    if (std::any_of(counts.begin(), counts.end(), [&](uint32_t c) { return c < k; })) {
        FSGPU_TRY(index_->fetch_live_host());
        const uint64_t need = std::min<uint64_t>(k, index_->live_count());
        for (uint32_t q = 0; q < nq; ++q)
            if (counts[q] < need) {
                flags[q] = counts[q] == 0 ? (uint32_t)FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS : (uint32_t)FSGPU_ANN_UNDERFILLED;
                under.push_back(q);
            }
    }
    if (!under.empty()) {
        const uint32_t nu = (uint32_t)under.size();
        std::vector<float> uq((size_t)nu * dim), us((size_t)nu * k);
        std::vector<uint32_t> ur((size_t)nu * k), uc(nu);
        for (uint32_t i = 0; i < nu; ++i) {
            if (on_device) FSGPU_HIP(hipMemcpy(uq.data() + (size_t)i * dim, queries + (size_t)under[i] * dim, (size_t)dim * 4, hipMemcpyDeviceToHost));
            else std::memcpy(uq.data() + (size_t)i * dim, queries + (size_t)under[i] * dim, (size_t)dim * 4);
        }
        FSGPU_TRY(index_->search_top_k_batched(uq.data(), nu, dim, k, nullptr, ur.data(), us.data(), uc.data(), nullptr));
        for (uint32_t i = 0; i < nu; ++i) {
            const uint32_t q = under[i];
            counts[q] = uc[i];
            if (on_device) {
                FSGPU_HIP(hipMemcpy(out_rows + (size_t)q * k, ur.data() + (size_t)i * k, (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_scores + (size_t)q * k, us.data() + (size_t)i * k, (size_t)k * 4, hipMemcpyHostToDevice));
                FSGPU_HIP(hipMemcpy(out_counts + q, &uc[i], 4, hipMemcpyHostToDevice));
            } else {
                std::memcpy(rows + (size_t)q * k, ur.data() + (size_t)i * k, (size_t)k * 4);
                std::memcpy(scores + (size_t)q * k, us.data() + (size_t)i * k, (size_t)k * 4);
            }
        }
    }
    for (uint32_t q = 0; q < nq; ++q) {
        if (flags[q] == FSGPU_ANN_UNDERFILLED) st.underfilled += 1;
        else if (flags[q] == FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS) st.empty_despite_indexed_points += 1;
        else st.approximate += 1;
    }
    if (on_device) {
        if (out_flags) FSGPU_HIP(hipMemcpy(out_flags, flags.data(), (size_t)nq * 4, hipMemcpyHostToDevice));
    } else {
        std::memcpy(out_rows, rows, hits);
        std::memcpy(out_scores, scores, hits);
        std::memcpy(out_counts, counts.data(), (size_t)nq * 4);
        if (out_flags) std::memcpy(out_flags, flags.data(), (size_t)nq * 4);
    }
    return done();
}

SearchError AnnIndex::certify_ef(const float* queries, uint32_t nq, const uint32_t* candidate_efs, uint32_t n_efs, uint32_t k, double target,
                                 double alpha, CertifiedEf* chosen, CertifiedEf* sweep, uint32_t* n_swept) {
    if (n_efs == 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "no candidate ef");
    std::vector<uint32_t> efs(candidate_efs, candidate_efs + n_efs);
    std::sort(efs.begin(), efs.end());
    efs.erase(std::unique(efs.begin(), efs.end()), efs.end());
    for (uint32_t ef : efs) FSGPU_TRY(check_call(k, ef));
    const uint32_t dim = index_->dimension();
    // the exact top-k is independent of ef: once per query
    std::vector<uint32_t> erows((size_t)nq * k), ecounts(nq, 0u), arows((size_t)nq * k), acounts(nq), aflags(nq);
    std::vector<float> escores((size_t)nq * k), ascores((size_t)nq * k);
    if (nq) FSGPU_TRY(index_->search_top_k_batched(queries, nq, dim, k, nullptr, erows.data(), escores.data(), ecounts.data(), nullptr));
    AnnStats sum;
    std::vector<double> recalls(nq);
    bool have_best = false;
    CertifiedEf best;
    uint32_t swept = 0;
    for (uint32_t ef : efs) {
        AnnStats st;
        FSGPU_TRY(search(queries, nq, dim, k, ef, arows.data(), ascores.data(), acounts.data(), aflags.data(), false, &st));
        sum.index_size = st.index_size;
        sum.dimension = st.dimension;
        sum.k_requested = k;
        sum.ef_search = std::max(sum.ef_search, ef);
        sum.launches += st.launches;
        sum.queries += st.queries;
        sum.approximate += st.approximate;
        sum.underfilled += st.underfilled;
        sum.empty_despite_indexed_points += st.empty_despite_indexed_points;
        sum.rows_scored += st.rows_scored;
        sum.steps += st.steps;
        sum.device_ms += st.device_ms;
        for (uint32_t q = 0; q < nq; ++q)
            recalls[q] = aflags[q] ? 0.0
                                   : recall_at_k_of_rows(arows.data() + (size_t)q * k, acounts[q], erows.data() + (size_t)q * k, ecounts[q]);
        CertifiedEf c;
        c.ef_search = ef;
        c.certified_recall = conformal_recall_lower_bound(recalls.data(), nq, alpha);
        c.meets_target = c.certified_recall >= target;
        sweep[swept++] = c;
        if (c.meets_target) {
            best = c;
            have_best = true;
            break;
        }
        if (!have_best || c.certified_recall > best.certified_recall) {
            best = c;
            have_best = true;
        }
    }
    last_ = sum;
    *chosen = best;
    *n_swept = swept;
    return ok();
}

}  // namespace fsgpu

// bert_reranker.cpp — the cross-encoder forward on one GPU (forward_batch, crates/frankensearch-rerank/src/native.rs:956-1130):
//   typed embeddings + LayerNorm (bert_rerank.hip)
//   layers 0 .. L-2: the embedder's fragment-order layer (QKV projection, per-pair attention, post-attention block)
//   layer L-1: QKV projection over every token, then ONLY the [CLS] rows (encoder_layer_cls, native.rs:628-700): the [CLS] query's
//              attention per pair and head (+ the gather of its residual row), the post-attention block over n_pairs rows
//   head: tanh pooler + 1-logit classifier + sigmoid (bert_rerank.hip)
// Every launch uses one kernel form fixed by the model's shape (the *_fixed launchers; the attention's per-pair work does not depend
// on the batch), so a pair's logit has the same bits alone, in a 100-pair call, in any order or chunk.
#include "bert_reranker.hpp"

#include <algorithm>
#include <cmath>
#include <string>

namespace fsgpu {

namespace {
SearchError rr_err(int32_t code, std::string detail) {
    SearchError e;
    e.code = code;
    e.detail = std::move(detail);
    return e;
}
#define RR_HIP(expr)                                                                                       \
    do {                                                                                                   \
        hipError_t _e = (expr);                                                                            \
        if (_e != hipSuccess) return rr_err(FSGPU_ERR_DEVICE, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)
#define RR_TRY(expr)             \
    do {                         \
        SearchError _s = (expr); \
        if (!_s.ok()) return _s; \
    } while (0)

SearchError upload(DeviceBuffer& dst, const float* src, size_t n) {
    if (!src) return rr_err(FSGPU_ERR_NULL_ARGUMENT, "missing reranker weight tensor");
    RR_TRY(dst.reserve(n * 4));
    RR_HIP(hipMemcpy(dst.ptr, src, n * 4, hipMemcpyHostToDevice));
    return SearchError{};
}
}  // namespace

SearchError NativeReranker::init(int device, const fsgpu_bert_config& cfg, const fsgpu_bert_weights& w, uint32_t type_vocab,
                                 const float* pooler_w, const float* pooler_b, const float* classifier_w, const float* classifier_b) {
    if (type_vocab == 0) return rr_err(FSGPU_ERR_INVALID_CONFIG, "type_vocab must be at least 1");
    if (!w.type_emb || !pooler_w || !pooler_b || !classifier_w || !classifier_b)
        return rr_err(FSGPU_ERR_NULL_ARGUMENT, "missing token-type, pooler or classifier weights");
    RR_TRY(enc_.init(device, cfg, w, FSGPU_BERT_LINEAR_F16));
    const int H = (int)cfg.hidden, I = (int)cfg.inter;
    if (!enc_.packed_ || !bert_post_attn_w_supported(H, I) || !bert_rerank_supported(H))
        return rr_err(FSGPU_ERR_INVALID_CONFIG, "the reranker needs the fragment-order layer (hidden 128 / 256 / 384, inter a multiple of 256)");
    type_vocab_ = type_vocab;
    RR_HIP(hipSetDevice(device));
    RR_TRY(upload(type_emb_, w.type_emb, (size_t)type_vocab * H));   // every token-type row (the embedder keeps row 0 only)
    RR_TRY(upload(pool_w_, pooler_w, (size_t)H * H));
    RR_TRY(upload(pool_b_, pooler_b, (size_t)H));
    RR_TRY(upload(cls_w_, classifier_w, (size_t)H));
    RR_TRY(upload(cls_b_, classifier_b, 1));
    return SearchError{};
}

SearchError NativeReranker::init_safetensors(int device, const void* blob, uint64_t blob_len, float ln_eps) {
    BertBlob b;
    RR_TRY(parse_bert_safetensors(blob, blob_len, ln_eps, &b));
    const uint64_t H = b.cfg.hidden;
    auto load_failed = [](const std::string& why) { return rr_err(FSGPU_ERR_MODEL_LOAD_FAILED, why); };
    auto find = [&](const std::string& key, const BlobTensor** t) -> SearchError {
        auto it = b.tensors.find(key);
        if (it == b.tensors.end()) return load_failed("missing tensor " + key);
        *t = &it->second;
        return SearchError{};
    };
    const BlobTensor *pw = nullptr, *pb = nullptr, *cw = nullptr, *cb = nullptr;
    RR_TRY(find("bert.pooler.dense.weight", &pw));
    RR_TRY(find("bert.pooler.dense.bias", &pb));
    RR_TRY(find("classifier.weight", &cw));
    RR_TRY(find("classifier.bias", &cb));
    if (pw->count != H * H) return load_failed("tensor bert.pooler.dense.weight holds " + std::to_string(pw->count) + " values, expected " + std::to_string(H * H));
    if (pb->count != H) return load_failed("tensor bert.pooler.dense.bias holds " + std::to_string(pb->count) + " values, expected " + std::to_string(H));
    if (cw->count == 0 || cw->count % H != 0)
        return load_failed("tensor classifier.weight holds " + std::to_string(cw->count) + " values, not a whole number of rows of " + std::to_string(H));
    const uint64_t rows = cw->count / H;
    if (rows != 1 || cb->count != 1)   // (forward_batch, native.rs:1122-1127: one logit per document)
        return load_failed("classifier: expected 1 logits, got " + std::to_string(rows > cb->count ? rows : cb->count) +
                           " (num_labels must be 1)");
    if (device < 0) return SearchError{};
    return init(device, b.cfg, b.w, b.type_rows, pw->data, pb->data, cw->data, cb->data);
}

// Pairs [p0, p1) of the compacted (non-empty) list = tokens [t0, t1) of the call's inputs; their chunk-relative offsets start at
// offs_[off_base].
SearchError NativeReranker::forward_chunk(uint32_t p0, uint32_t p1, uint32_t t0, uint32_t t1, uint32_t max_seq, uint32_t off_base) {
    const int H = (int)enc_.cfg_.hidden, T = (int)(t1 - t0), n = (int)(p1 - p0);
    const uint32_t total = (uint32_t)(in_host_.size() / 3);
    hipStream_t stream = enc_.stream_;
    const int32_t* in = static_cast<const int32_t*>(in_.ptr);
    const uint32_t* offs = static_cast<const uint32_t*>(offs_.ptr) + off_base;
    float* x = static_cast<float*>(x_.ptr);
    _Float16* xh = static_cast<_Float16*>(xh_.ptr);
    _Float16* qkv = static_cast<_Float16*>(qkv_.ptr);
    _Float16* ctx = static_cast<_Float16*>(ctx_.ptr);
    float* xc = static_cast<float*>(xc_.ptr);
    _Float16* xch = static_cast<_Float16*>(xch_.ptr);
    _Float16* ctxc = static_cast<_Float16*>(ctxc_.ptr);
    RR_HIP(launch_bert_embed_typed_ln(in + t0, in + total + t0, in + 2 * (size_t)total + t0, static_cast<const float*>(enc_.word_.ptr),
                                      static_cast<const float*>(enc_.pos_.ptr), static_cast<const float*>(type_emb_.ptr),
                                      static_cast<const float*>(enc_.emb_ln_w_.ptr), static_cast<const float*>(enc_.emb_ln_b_.ptr), x, xh,
                                      T, H, enc_.cfg_.ln_eps, stream));
    const float scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    const size_t L = enc_.layers_.size();
    for (size_t li = 0; li + 1 < L; ++li) {
        const NativeEmbedder::Layer& l = enc_.layers_[li];
        RR_TRY(enc_.packed_qkv(l, xh, qkv, T, true, stream));
        RR_HIP(launch_bert_attention_h(qkv, offs, ctx, n, (int)enc_.cfg_.heads, H, (int)max_seq, scale, stream));
        RR_TRY(enc_.packed_post_attention(l, ctx, x, xh, T, true, stream));
    }
    const NativeEmbedder::Layer& last = enc_.layers_[L - 1];
    RR_TRY(enc_.packed_qkv(last, xh, qkv, T, true, stream));
    RR_HIP(launch_bert_cls_attention(qkv, offs, x, ctxc, xc, n, (int)enc_.cfg_.heads, H, scale, stream));
    RR_TRY(enc_.packed_post_attention(last, ctxc, xc, xch, n, true, stream));
    RR_HIP(launch_bert_cls_head(xc, static_cast<const float*>(pool_w_.ptr), static_cast<const float*>(pool_b_.ptr),
                                static_cast<const float*>(cls_w_.ptr), static_cast<const float*>(cls_b_.ptr),
                                static_cast<float*>(logits_.ptr) + p0, static_cast<float*>(scores_.ptr) + p0, n, H, stream));
    return SearchError{};
}

SearchError NativeReranker::score(const int32_t* ids, const int32_t* type_ids, const uint32_t* offsets, uint32_t n, float* logits,
                                  float* scores) {
    return score_any(ids, type_ids, false, offsets, n, logits, scores);
}

SearchError NativeReranker::score_device_ids(const int32_t* ids_dev, const int32_t* type_ids_dev, const uint32_t* offsets, uint32_t n,
                                             float* logits, float* scores) {
    return score_any(ids_dev, type_ids_dev, true, offsets, n, logits, scores);
}

// on_device: ids / type_ids are device memory, never read on the host (their ranges are the caller's word), starting at pair 0's
// first token, and no pair is empty — so the live pairs' tokens are the call's tokens, in place.
SearchError NativeReranker::score_any(const int32_t* ids, const int32_t* type_ids, bool on_device, const uint32_t* offsets, uint32_t n,
                                      float* logits, float* scores) {
    if (n == 0) return SearchError{};
    if (!offsets || !logits || !scores) return rr_err(FSGPU_ERR_NULL_ARGUMENT, "offsets/out_logits/out_scores is null");
    std::lock_guard<std::mutex> lock(mu_);
    const uint32_t max_len = max_length(), vocab = enc_.cfg_.vocab;
    // the non-empty pairs, validated before anything is launched (an empty pair is logit 0 / score 0.5, forward_batch native.rs:959-961)
    std::vector<uint32_t> live;
    uint64_t total64 = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return rr_err(FSGPU_ERR_INVALID_CONFIG, "offsets must be non-decreasing");
        const uint32_t len = offsets[i + 1] - offsets[i];
        if (len > max_len)
            return rr_err(FSGPU_ERR_INVALID_CONFIG, "pair longer than max_position_embeddings (" + std::to_string(len) + " > " +
                                                        std::to_string(max_len) + " tokens: truncate first)");
        if (len == 0 && on_device) return rr_err(FSGPU_ERR_INVALID_CONFIG, "an empty pair in a device CSR");
        if (len == 0) continue;
        if (!ids || !type_ids) return rr_err(FSGPU_ERR_NULL_ARGUMENT, "ids/type_ids is null");
        for (uint32_t t = offsets[i]; t < offsets[i + 1] && !on_device; ++t) {
            if (ids[t] < 0 || (uint32_t)ids[t] >= vocab) return rr_err(FSGPU_ERR_INVALID_CONFIG, "token id out of vocabulary");
            if (type_ids[t] < 0 || (uint32_t)type_ids[t] >= type_vocab_)
                return rr_err(FSGPU_ERR_INVALID_CONFIG, "token type id out of range (type_vocab_size " + std::to_string(type_vocab_) + ")");
        }
        live.push_back(i);
        total64 += len;
    }
    for (uint32_t i = 0; i < n; ++i) {
        logits[i] = 0.0f;
        scores[i] = 0.5f;
    }
    if (live.empty()) return SearchError{};
    const uint32_t total = (uint32_t)total64, m = (uint32_t)live.size();
    // inputs: ids | types | positions of the live pairs, concatenated; chunks of whole pairs within kChunkTokens tokens
    in_host_.resize((size_t)3 * total);
    struct Chunk {
        uint32_t p0, p1, t0, t1, max_seq, off_base;
    };
    std::vector<Chunk> chunks;
    offs_host_.clear();
    uint32_t t = 0;
    for (uint32_t k = 0; k < m; ++k) {
        const uint32_t i = live[k], len = offsets[i + 1] - offsets[i];
        if (chunks.empty() || chunks.back().t1 - chunks.back().t0 + len > kChunkTokens) {
            chunks.push_back(Chunk{k, k, t, t, 0, (uint32_t)offs_host_.size()});
            offs_host_.push_back(0);
        }
        Chunk& c = chunks.back();
        for (uint32_t j = 0; j < len; ++j) {
            if (!on_device) {
                in_host_[t + j] = ids[offsets[i] + j];
                in_host_[(size_t)total + t + j] = type_ids[offsets[i] + j];
            }
            in_host_[2 * (size_t)total + t + j] = (int32_t)j;   // positions restart at 0 per pair
        }
        t += len;
        c.p1 = k + 1;
        c.t1 = t;
        if (len > c.max_seq) c.max_seq = len;
        offs_host_.push_back(t - c.t0);
    }
    uint32_t chunk_tokens = 0, chunk_pairs = 0;
    for (const Chunk& c : chunks) {
        chunk_tokens = std::max(chunk_tokens, c.t1 - c.t0);
        chunk_pairs = std::max(chunk_pairs, c.p1 - c.p0);
    }
    const size_t H = enc_.cfg_.hidden;
    RR_HIP(hipSetDevice(enc_.device_));
    RR_TRY(in_.reserve(in_host_.size() * 4));
    RR_TRY(offs_.reserve(offs_host_.size() * 4));
    RR_TRY(logits_.reserve((size_t)m * 4));
    RR_TRY(scores_.reserve((size_t)m * 4));
    RR_TRY(x_.reserve((size_t)chunk_tokens * H * 4));
    RR_TRY(xh_.reserve((size_t)chunk_tokens * H * 2));
    RR_TRY(qkv_.reserve((size_t)chunk_tokens * 3 * H * 2));
    RR_TRY(ctx_.reserve((size_t)chunk_tokens * H * 2));
    RR_TRY(xc_.reserve((size_t)chunk_pairs * H * 4));
    RR_TRY(xch_.reserve((size_t)chunk_pairs * H * 2));
    RR_TRY(ctxc_.reserve((size_t)chunk_pairs * H * 2));
    hipStream_t stream = enc_.stream_;
    if (on_device) {   // ids | types from where they lie, positions from the host
        int32_t* in = static_cast<int32_t*>(in_.ptr);
        RR_HIP(hipMemcpyAsync(in, ids + offsets[0], (size_t)total * 4, hipMemcpyDeviceToDevice, stream));
        RR_HIP(hipMemcpyAsync(in + total, type_ids + offsets[0], (size_t)total * 4, hipMemcpyDeviceToDevice, stream));
        RR_HIP(hipMemcpyAsync(in + 2 * (size_t)total, in_host_.data() + 2 * (size_t)total, (size_t)total * 4, hipMemcpyHostToDevice, stream));
    } else {
        RR_HIP(hipMemcpyAsync(in_.ptr, in_host_.data(), in_host_.size() * 4, hipMemcpyHostToDevice, stream));
    }
    RR_HIP(hipMemcpyAsync(offs_.ptr, offs_host_.data(), offs_host_.size() * 4, hipMemcpyHostToDevice, stream));
    for (const Chunk& c : chunks) RR_TRY(forward_chunk(c.p0, c.p1, c.t0, c.t1, c.max_seq, c.off_base));
    std::vector<float> lg(m), sc(m);
    RR_HIP(hipMemcpyAsync(lg.data(), logits_.ptr, (size_t)m * 4, hipMemcpyDeviceToHost, stream));
    RR_HIP(hipMemcpyAsync(sc.data(), scores_.ptr, (size_t)m * 4, hipMemcpyDeviceToHost, stream));
    RR_HIP(hipStreamSynchronize(stream));
    for (uint32_t k = 0; k < m; ++k) {
        logits[live[k]] = lg[k];
        scores[live[k]] = sc[k];
    }
    return SearchError{};
}

}  // namespace fsgpu

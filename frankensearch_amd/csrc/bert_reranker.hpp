// bert_reranker.hpp — host side of the GPU cross-encoder; mirrors the reference's NativeReranker
// (crates/frankensearch-rerank/src/native.rs:1240, rerank_sync :1636-1710): a BertForSequenceClassification with one logit over
// `[CLS] query [SEP] doc [SEP]` pairs that the caller has tokenised and truncated.
#pragma once

#include <cstdint>
#include <mutex>
#include <vector>

#include "bert_embedder.hpp"

namespace fsgpu {

class NativeReranker {
  public:
    // The encoder's tensors as fsgpu_bert_weights (type_emb: [type_vocab, hidden]), plus the pooler ([hidden, hidden] + [hidden]) and
    // the one-row classifier ([1, hidden] + [1]), all f32 in HuggingFace layout.
    SearchError init(int device, const fsgpu_bert_config& cfg, const fsgpu_bert_weights& w, uint32_t type_vocab, const float* pooler_w,
                     const float* pooler_b, const float* classifier_w, const float* classifier_b);
    // parse_weights' contract (native.rs:1359-1602) plus bert.pooler.dense.{weight,bias} and classifier.{weight,bias}; device < 0
    // validates the blob only.
    SearchError init_safetensors(int device, const void* blob, uint64_t blob_len, float ln_eps);
    // Pair i is ids[offsets[i]..offsets[i+1]) with type_ids alongside; logits / scores [n].  A zero-length pair gets logit 0, score 0.5.
    SearchError score(const int32_t* ids, const int32_t* type_ids, const uint32_t* offsets, uint32_t n, float* logits, float* scores);
    // ... over ids and type ids that already lie in this reranker's device memory (the device tokenizer's pair CSR: every id below
    // vocab(), every type id 0 or 1, no empty pair); offsets stay a host array.  The same chunks and kernels as score(), so the
    // same bits: the chain reads device-to-device copies of the ids and type ids.
    SearchError score_device_ids(const int32_t* ids_dev, const int32_t* type_ids_dev, const uint32_t* offsets, uint32_t n, float* logits,
                                 float* scores);
    uint32_t vocab() const { return enc_.cfg_.vocab; }
    uint32_t type_vocab() const { return type_vocab_; }
    int device() const { return enc_.device(); }
    uint32_t max_length() const { return enc_.cfg_.max_pos; }   // min(max_position_embeddings, 512)

    // Tokens per forward: a call runs its pairs in consecutive chunks of at most this many tokens.  Every kernel of the chain keeps
    // one form whatever the chunk's size (launch_bert_*_fixed), so the chunking changes no bit of a pair's logit.
    static constexpr uint32_t kChunkTokens = 16384;

  private:
    SearchError score_any(const int32_t* ids, const int32_t* type_ids, bool on_device, const uint32_t* offsets, uint32_t n, float* logits,
                          float* scores);
    SearchError forward_chunk(uint32_t p0, uint32_t p1, uint32_t t0, uint32_t t1, uint32_t max_seq, uint32_t off_base);

    std::mutex mu_;          // one caller at a time (native.rs:1668)
    NativeEmbedder enc_;     // the encoder's weights (f16 + fragment order), its stream and its layer steps
    uint32_t type_vocab_ = 0;
    DeviceBuffer type_emb_, pool_w_, pool_b_, cls_w_, cls_b_;
    // per call: the non-empty pairs' ids | types | positions, each chunk's offsets (relative to the chunk), logits, scores
    DeviceBuffer in_, offs_, logits_, scores_;
    // per chunk: the layer chain's workspaces (x f32 / f16, Q|K|V f16, context f16) and the [CLS] rows of the last layer
    DeviceBuffer x_, xh_, qkv_, ctx_, xc_, xch_, ctxc_;
    std::vector<int32_t> in_host_;
    std::vector<uint32_t> offs_host_;
};

}  // namespace fsgpu

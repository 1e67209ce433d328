// bert_embedder.hpp — host side of the GPU MiniLM-class embedder; mirrors the reference's NativeEmbedder
// (crates/frankensearch-rerank/src/native_embedder.rs:40-50,173-255: embed_sync / embed_batch_sync over token
// ids) and the weight contract of parse_weights (crates/frankensearch-rerank/src/native.rs:1359-1602).
#pragma once

#include <cstdint>
#include <deque>
#include <map>
#include <string>
#include <mutex>
#include <tuple>
#include <vector>

#include "../../include/fsgpu.h"
#include "vector_index.hpp"

namespace fsgpu {

// A safetensors blob in HuggingFace key layout, parsed in place (safetensors.cpp; parse_weights, native.rs:1359-1602): the encoder's
// shape and tensors, and every F32 tensor by its `bert.`-normalised key (the reranker's pooler / classifier are looked up there).
struct BlobTensor {
    const float* data = nullptr;
    std::vector<uint64_t> shape;
    uint64_t count = 0;
};
struct BertBlob {
    fsgpu_bert_config cfg{};
    fsgpu_bert_weights w{};
    uint32_t type_rows = 0;
    std::vector<fsgpu_bert_layer_weights> layers;
    std::map<std::string, BlobTensor> tensors;
    std::deque<std::vector<float>> staged;   // copies of tensors that were not 4-byte aligned in the blob
};
SearchError parse_bert_safetensors(const void* blob, uint64_t blob_len, float ln_eps, BertBlob* out);

// The row blocks of the one-launch forward of short texts (bert_docs_w.hip): consecutive texts packed greedily into blocks of at most
// 32 tokens, a block never splitting a text, and each block's 32 rows laid out so that it needs ONE read of the inputs: token id (-1 =
// padding), rows of the block << 16 | position inside the text << 8 | the text's index among the block's non-empty texts.  The call's
// single input block is [offsets | blk_tok | blk_doc | row_id | row_meta], in_bytes long (a multiple of 256).
struct BertDocsPacking {
    uint32_t n = 0, nblocks = 0;
    std::vector<uint32_t> blk_tok, blk_doc, row_meta;
    std::vector<int32_t> row_id;
    size_t o_tok = 0, o_doc = 0, o_rid = 0, o_rmeta = 0, in_bytes = 0;
    void fill(unsigned char* dst, const uint32_t* offs) const;           // the input block, for the offsets it was packed from
    void point(BertDocsArgs& a, const unsigned char* base) const;        // the kernel's five input pointers into a copy at `base`
};
// ids: the call's tokens (null: every row id is left at -1, for a caller that fills them on the device); offs [n + 1]: the call's
// offsets rebased to 0, every text at most 32 tokens; total = offs[n]
BertDocsPacking bert_docs_pack(const int32_t* ids, const uint32_t* offs, uint32_t n, uint32_t total);

class NativeEmbedder {
  public:
    ~NativeEmbedder();
    // linear_format: FSGPU_BERT_LINEAR_F16 (f16 matrix-core linears) or FSGPU_BERT_LINEAR_INT8_DYNAMIC (bert_int8.hip: int8
    // per-output-channel weights, per-row dynamic int8 activations — the arithmetic of the reference's native forward).
    SearchError init(int device, const fsgpu_bert_config& cfg, const fsgpu_bert_weights& w,
                     uint32_t linear_format = FSGPU_BERT_LINEAR_F16);
    // NativeEmbedder::load's weight contract: a safetensors blob in HuggingFace key layout (safetensors.cpp; parse_weights,
    // crates/frankensearch-rerank/src/native.rs:1359-1602).  device < 0 validates the blob only.
    SearchError init_safetensors(int device, const void* blob, uint64_t blob_len, float ln_eps,
                                 uint32_t linear_format = FSGPU_BERT_LINEAR_F16);
    // ids: concatenated token ids; text i owns ids[offsets[i]..offsets[i+1]).  out: [n, hidden] f32.
    // out_dev (on this embedder's device, may be null): the pooled vectors are left in device memory — the hand-off to a search that
    // takes device queries; out (may then be null): the host copy.  Either way the call returns when the forward has finished.
    SearchError embed_batch(const int32_t* ids, const uint32_t* offsets, uint32_t n, float* out, float* out_dev = nullptr);
    // ... over ids that already lie in this embedder's device memory (the device tokenizer's CSR, every id below vocab()); offsets
    // stay a host array.  The same kernels in the same forms as embed_batch, so the same bits: the row blocks of the short-text
    // forward are filled from the device ids by a kernel, the other forwards read a device-to-device copy; no pinned block, no graph.
    SearchError embed_batch_device_ids(const int32_t* ids_dev, const uint32_t* offsets, uint32_t n, float* out, float* out_dev);
    uint32_t vocab() const { return cfg_.vocab; }
    uint32_t dimension() const { return cfg_.hidden; }
    int device() const { return device_; }
    uint32_t linear_format() const { return int8_ ? FSGPU_BERT_LINEAR_INT8_DYNAMIC : FSGPU_BERT_LINEAR_F16; }

  private:
    struct Layer {
        DeviceBuffer qkv_w, ao_w, i_w, o_w;              // f16 [N,K]
        DeviceBuffer qkv_wp, ao_wp, i_wp, o_wp;          // the same weights in matrix-core fragment order (bert_gemm_w.hip)
        DeviceBuffer qkv_b, ao_b, ln1_w, ln1_b, i_b, o_b, ln2_w, ln2_b;  // f32
        DeviceBuffer qkv_q, ao_q, i_q, o_q;              // int8 mode: fragment-order int8 codes (bert_i8_pack_w_kernel)
        DeviceBuffer qkv_s, ao_s, i_s, o_s;              // int8 mode: f32 scale per output channel
    };
    SearchError upload_f32(DeviceBuffer& dst, const float* src, size_t n);
    SearchError upload_f16(DeviceBuffer& dst, const float* src, size_t n, DeviceBuffer& staging);
    SearchError pack_weights(DeviceBuffer& dst, const DeviceBuffer& src, int N, int K);
    SearchError upload_i8(DeviceBuffer& q, DeviceBuffer& s, const float* src, int N, int K, DeviceBuffer& staging);
    SearchError forward(uint32_t n_docs, uint32_t tokens, uint32_t max_seq);
    // the fragment-order batch path over texts [d0, d1) = tokens [t0, t1) on `stream` (bert_gemm_w.hip)
    SearchError forward_packed_range(uint32_t d0, uint32_t d1, uint32_t t0, uint32_t t1, uint32_t max_seq, hipStream_t stream);
    // int8 mode: ONE per-layer chain for every batch shape (bert_int8.hip + the f32-operand attention), so a text's vector has the
    // same bits whatever batch it rides in
    SearchError forward_int8(uint32_t n_docs, uint32_t tokens, uint32_t max_seq);
    SearchError forward_query(uint32_t n_docs, uint32_t tokens);   // <= 32 tokens: 25 launches (bert_query_kernels.hip)
    bool query_path(uint32_t tokens) const;
    bool one_launch_path() const;                                  // ... as ONE launch with grid-wide barriers (experiments builds)
    bool docs_path(uint32_t tokens, uint32_t max_seq) const;       // every text <= 32 tokens: ONE launch (bert_docs_w.hip)
    SearchError embed_docs(const int32_t* ids, const std::vector<uint32_t>& offs, uint32_t n, uint32_t total, float* out, float* out_dev,
                           bool ids_on_device);
    SearchError embed_any(const int32_t* ids, bool ids_on_device, const uint32_t* offsets, uint32_t n, float* out, float* out_dev);
    SearchError reserve_workspaces(uint32_t tokens);
    void drop_graphs();
    // One layer of the fragment-order path, in pieces its callers share: the QKV projection of T rows (f16 Q | K | V out), then — after
    // the caller's attention — the post-attention block over M rows (output projection + LN, FFN + LN).  fixed: the launchers that keep
    // ONE kernel form whatever the row count (launch_bert_*_fixed): the cross-encoder's chain (bert_reranker.cpp)
    SearchError packed_qkv(const Layer& l, const _Float16* x_h, _Float16* qkv, int T, bool fixed, hipStream_t stream);
    SearchError packed_post_attention(const Layer& l, const _Float16* ctx, float* x, _Float16* x_h, int M, bool fixed, hipStream_t stream);
    friend class NativeReranker;   // the cross-encoder runs this embedder's uploaded weights, stream and layer steps

    std::mutex mu_;
    int device_ = -1;
    fsgpu_bert_config cfg_{};
    hipStream_t stream_ = nullptr;
    DeviceBuffer word_, pos_, type_, emb_ln_w_, emb_ln_b_;
    std::vector<Layer> layers_;
    // workspaces
    DeviceBuffer ids_, positions_, offsets_, x_f32_, x_h_, qkv_f32_, ctx_h_, tmp_f32_, inter_h_, out_, q_x_, q_parts_;
    bool int8_ = false;                 // FSGPU_BERT_LINEAR_INT8_DYNAMIC
    DeviceBuffer qx_, sx_, inter_f32_;  // int8 mode: a linear's input codes [T, max(H, I)] and row scales [T]; the GELU output f32
    // pinned staging for small calls (see embed_batch)
    static constexpr size_t kPinnedIoBytes = 512 * 1024;
    void* io_host_ = nullptr;
    bool io_failed_ = false;
    float* pooled_out_ = nullptr;  // where the pool kernel writes during a pinned call
    const int32_t *q_ids_ = nullptr, *q_positions_ = nullptr;  // query path of a pinned call: inputs read in place
    const uint32_t* q_offsets_ = nullptr;
    // the one-launch query forward: the stage table on the device (+ the host copies it was sent from / is compared with), the
    // barrier counter, how many launches have used it, the mapped word a block raises when a barrier wait gave up
    DeviceBuffer q_stages_, q_counter_;
    std::vector<BertQueryArgs> q_stages_host_[2];
    std::vector<unsigned char> q_kinds_host_[2];
    int q_stages_flip_ = 0;
    unsigned int q_launches_ = 0;
    unsigned int* q_status_ = nullptr;
    bool q_one_launch_ok_ = true;
    // Query-sized calls replay a captured hipGraph of the whole call (three H2D copies + the ~44 kernels of the forward):
    // the chain is launch-bound, and a replay costs one submission instead of one per kernel.  One graph per call shape
    // (texts, tokens, longest text), built the second time a shape is seen; every buffer a graph names is allocated at its
    // graph-eligible maximum up front, and the graphs are dropped if a larger call ever moves one.
    struct GraphEntry {
        hipGraphExec_t exec = nullptr;
        uint32_t seen = 0;
    };
    static constexpr uint32_t kGraphMaxTokens = 8192;
    static constexpr size_t kGraphMaxEntries = 128;
    std::map<std::tuple<uint32_t, uint32_t, uint32_t>, GraphEntry> graphs_;
    bool graphs_enabled_ = true;
    bool packed_ = false;  // every layer has its fragment-order copies: the batch path runs bert_gemm_w.hip
    DeviceBuffer docs_layers_, docs_in_, docs_out_;   // bert_docs_w.hip: the layers' pointer table; inputs of a call too large for the pinned block
    bool docs_ready_ = false;
    static constexpr size_t kDocsIoBytes = 2 * 1024 * 1024;   // pinned block of the one-launch path: row tables in, pooled vectors out
    void* docs_io_ = nullptr;
    bool docs_io_failed_ = false;
};

}  // namespace fsgpu

// bert_embedder.cpp — orchestration of the BERT forward on one GPU (see bert_kernels.hip for the arithmetic).
// Layer order follows encoder_layer_raw (crates/frankensearch-rerank/src/native.rs:587-626).
#include "lab_env.hpp"
#include "bert_embedder.hpp"
#include "wordpiece.hpp"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

// rows (tokens) from which the batch path runs the post-attention block as three launches with a weight-stationary FFN-up GEMM
// instead of the fused bert_ffn_w_kernel.  OFF by default: on 32 x 512 tokens the three launches measured 1.440 ms against the fused
// kernel's 1.153 ms (profiles/r04/enc_large_m_ab.txt) — the intermediate's round trip through HBM costs more than the
// weight-stationary GEMM saves.  Kept for A/B builds (-DFSGPU_BERT_SPLIT_MIN_TOKENS=6144).
#ifndef FSGPU_BERT_SPLIT_MIN_TOKENS
#define FSGPU_BERT_SPLIT_MIN_TOKENS (1 << 30)
#endif

namespace fsgpu {

namespace {
SearchError err(int32_t code, std::string detail) {
    SearchError e;
    e.code = code;
    e.detail = std::move(detail);
    return e;
}
SearchError hip_err(hipError_t e, const char* what) {
    return err(FSGPU_ERR_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}
#define BERT_HIP(expr)                                   \
    do {                                                 \
        hipError_t _e = (expr);                          \
        if (_e != hipSuccess) return hip_err(_e, #expr); \
    } while (0)
#define BERT_TRY(expr)           \
    do {                         \
        SearchError _s = (expr); \
        if (!_s.ok()) return _s; \
    } while (0)
}  // namespace

NativeEmbedder::~NativeEmbedder() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    drop_graphs();
    if (stream_) (void)hipStreamDestroy(stream_);
    if (io_host_) (void)hipHostFree(io_host_);
    if (q_status_) (void)hipHostFree(q_status_);
    if (docs_io_) (void)hipHostFree(docs_io_);
    for (DeviceBuffer* b : {&word_, &pos_, &type_, &emb_ln_w_, &emb_ln_b_, &ids_, &positions_, &offsets_, &x_f32_, &x_h_,
                            &qkv_f32_, &ctx_h_, &tmp_f32_, &inter_h_, &out_, &q_x_, &q_parts_, &q_stages_, &q_counter_, &docs_layers_, &docs_in_, &docs_out_,
                            &qx_, &sx_, &inter_f32_})
        b->release();
    for (Layer& l : layers_)
        for (DeviceBuffer* b : {&l.qkv_w, &l.ao_w, &l.i_w, &l.o_w, &l.qkv_wp, &l.ao_wp, &l.i_wp, &l.o_wp, &l.qkv_b, &l.ao_b, &l.ln1_w, &l.ln1_b, &l.i_b, &l.o_b,
                                &l.ln2_w, &l.ln2_b, &l.qkv_q, &l.ao_q, &l.i_q, &l.o_q, &l.qkv_s, &l.ao_s, &l.i_s, &l.o_s})
            b->release();
}

SearchError NativeEmbedder::upload_f32(DeviceBuffer& dst, const float* src, size_t n) {
    if (!src) return err(FSGPU_ERR_NULL_ARGUMENT, "missing weight tensor");
    BERT_TRY(dst.reserve(n * 4));
    BERT_HIP(hipMemcpy(dst.ptr, src, n * 4, hipMemcpyHostToDevice));
    return SearchError{};
}

SearchError NativeEmbedder::upload_f16(DeviceBuffer& dst, const float* src, size_t n, DeviceBuffer& staging) {
    if (!src) return err(FSGPU_ERR_NULL_ARGUMENT, "missing weight tensor");
    BERT_TRY(staging.reserve(n * 4));
    BERT_TRY(dst.reserve(n * 2));
    BERT_HIP(hipMemcpy(staging.ptr, src, n * 4, hipMemcpyHostToDevice));
    BERT_HIP(launch_bert_to_half(static_cast<const float*>(staging.ptr), dst.ptr, n, nullptr));
    BERT_HIP(hipDeviceSynchronize());
    return SearchError{};
}

SearchError NativeEmbedder::pack_weights(DeviceBuffer& dst, const DeviceBuffer& src, int N, int K) {
    BERT_TRY(dst.reserve((size_t)N * K * 2));
    BERT_HIP(launch_bert_pack_w(src.ptr, dst.ptr, N, K, nullptr));
    return SearchError{};
}

// int8 mode (bert_int8.hip): W [N, K] f32 -> the per-output-channel codes in fragment order + their scales, quantised on the device
SearchError NativeEmbedder::upload_i8(DeviceBuffer& q, DeviceBuffer& s, const float* src, int N, int K, DeviceBuffer& staging) {
    if (!src) return err(FSGPU_ERR_NULL_ARGUMENT, "missing weight tensor");
    BERT_TRY(staging.reserve((size_t)N * K * 4));
    BERT_TRY(q.reserve(bert_i8_packed_bytes(N, K)));
    BERT_TRY(s.reserve((size_t)N * 4));
    BERT_HIP(hipMemcpy(staging.ptr, src, (size_t)N * K * 4, hipMemcpyHostToDevice));
    BERT_HIP(launch_bert_i8_pack_w(static_cast<const float*>(staging.ptr), q.ptr, static_cast<float*>(s.ptr), N, K, nullptr));
    BERT_HIP(hipDeviceSynchronize());   // (the staging buffer is refilled by the next tensor)
    return SearchError{};
}

SearchError NativeEmbedder::init(int device, const fsgpu_bert_config& cfg, const fsgpu_bert_weights& w, uint32_t linear_format) {
    if (cfg.hidden == 0 || cfg.hidden % 128 != 0 || cfg.hidden > 1024)
        return err(FSGPU_ERR_INVALID_CONFIG, "hidden must be a multiple of 128 and <= 1024");
    if (cfg.heads * 32 != cfg.hidden) return err(FSGPU_ERR_INVALID_CONFIG, "head dimension must be 32");
    if (cfg.inter == 0 || cfg.inter % 128 != 0) return err(FSGPU_ERR_INVALID_CONFIG, "inter must be a multiple of 128");
    if (cfg.layers == 0 || cfg.vocab == 0 || cfg.max_pos == 0 || cfg.max_pos > 512)
        return err(FSGPU_ERR_INVALID_CONFIG, "layers/vocab must be non-zero and max_pos in 1..=512");
    if (linear_format != FSGPU_BERT_LINEAR_F16 && linear_format != FSGPU_BERT_LINEAR_INT8_DYNAMIC)
        return err(FSGPU_ERR_INVALID_CONFIG, "unknown linear format");
    const bool int8 = linear_format == FSGPU_BERT_LINEAR_INT8_DYNAMIC;
    if (int8 && !(bert_i8_gemm_supported(3 * (int)cfg.hidden, (int)cfg.hidden) && bert_i8_gemm_supported((int)cfg.inter, (int)cfg.hidden) &&
                  bert_i8_gemm_supported((int)cfg.hidden, (int)cfg.inter)))
        return err(FSGPU_ERR_INVALID_CONFIG, "int8 linears need hidden and inter to be multiples of 64");
    if (!w.layers) return err(FSGPU_ERR_NULL_ARGUMENT, "layer weights are null");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return err(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (device < 0 || device >= count) return err(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
    BERT_HIP(hipSetDevice(device));
    device_ = device;
    cfg_ = cfg;
    int8_ = int8;
    {
        // The encoder is a chain of short kernels; a scan on another stream is a few long, chip-filling ones.  With equal
        // priority the chain queues behind every scan launch (two-tier load, 1,024 callers: 44 k -> 48 k queries/s and
        // phase-0 p50 9.5 -> 5.6 ms with the encoders' streams at the highest priority).
        int least = 0, greatest = 0;
        BERT_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        BERT_HIP(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest));
    }
    const size_t H = cfg.hidden, I = cfg.inter;
    BERT_TRY(upload_f32(word_, w.word_emb, (size_t)cfg.vocab * H));
    BERT_TRY(upload_f32(pos_, w.pos_emb, (size_t)cfg.max_pos * H));
    BERT_TRY(upload_f32(type_, w.type_emb, H));  // token type 0 only (single text, native.rs:1166)
    BERT_TRY(upload_f32(emb_ln_w_, w.emb_ln_w, H));
    BERT_TRY(upload_f32(emb_ln_b_, w.emb_ln_b, H));
    DeviceBuffer staging;
    layers_.resize(cfg.layers);
    for (uint32_t i = 0; i < cfg.layers; ++i) {
        const fsgpu_bert_layer_weights& lw = w.layers[i];
        Layer& l = layers_[i];
        // Q/K/V stacked to [3H, H] (parse_weights, native.rs:1500-1540)
        if (!lw.q_w || !lw.k_w || !lw.v_w || !lw.q_b || !lw.k_b || !lw.v_b) {
            staging.release();
            return err(FSGPU_ERR_NULL_ARGUMENT, "missing q/k/v weights");
        }
        std::vector<float> stacked(3 * H * H), sb(3 * H);
        std::copy(lw.q_w, lw.q_w + H * H, stacked.begin());
        std::copy(lw.k_w, lw.k_w + H * H, stacked.begin() + H * H);
        std::copy(lw.v_w, lw.v_w + H * H, stacked.begin() + 2 * H * H);
        std::copy(lw.q_b, lw.q_b + H, sb.begin());
        std::copy(lw.k_b, lw.k_b + H, sb.begin() + H);
        std::copy(lw.v_b, lw.v_b + H, sb.begin() + 2 * H);
        // int8 mode: the fused [3H, H] QKV linear is quantised per output channel as one matrix (native.rs:1546-1600); no f16 copies
        SearchError e = int8 ? upload_i8(l.qkv_q, l.qkv_s, stacked.data(), (int)(3 * H), (int)H, staging)
                             : upload_f16(l.qkv_w, stacked.data(), stacked.size(), staging);
        if (e.ok()) e = upload_f32(l.qkv_b, sb.data(), sb.size());
        if (e.ok()) e = int8 ? upload_i8(l.ao_q, l.ao_s, lw.ao_w, (int)H, (int)H, staging) : upload_f16(l.ao_w, lw.ao_w, H * H, staging);
        if (e.ok()) e = upload_f32(l.ao_b, lw.ao_b, H);
        if (e.ok()) e = upload_f32(l.ln1_w, lw.ln1_w, H);
        if (e.ok()) e = upload_f32(l.ln1_b, lw.ln1_b, H);
        if (e.ok()) e = int8 ? upload_i8(l.i_q, l.i_s, lw.i_w, (int)I, (int)H, staging) : upload_f16(l.i_w, lw.i_w, I * H, staging);
        if (e.ok()) e = upload_f32(l.i_b, lw.i_b, I);
        if (e.ok()) e = int8 ? upload_i8(l.o_q, l.o_s, lw.o_w, (int)H, (int)I, staging) : upload_f16(l.o_w, lw.o_w, H * I, staging);
        if (e.ok()) e = upload_f32(l.o_b, lw.o_b, H);
        if (e.ok()) e = upload_f32(l.ln2_w, lw.ln2_w, H);
        if (e.ok()) e = upload_f32(l.ln2_b, lw.ln2_b, H);
        if (!e.ok()) {
            staging.release();
            return e;
        }
    }
    staging.release();
    if (int8) return SearchError{};   // (the f16 paths below — fragment-order copies, the one-launch table — are not used)
    // Fragment-order copies for the batch path (bert_gemm_w.hip): +2 bytes per weight (22 MB for MiniLM-L6).
    // FSGPU_BERT_GEMM_V1 keeps the LDS-tiled kernels of bert_kernels.hip (A/B runs).
    const int Hi = (int)H, Ii = (int)I;
    if (!fsgpu::lab_env("FSGPU_BERT_GEMM_V1") && bert_gemm_w_supported(3 * Hi, Hi) && bert_gemm_w_supported(Ii, Hi) &&
        bert_gemm_ln_w_supported(Hi, Hi) && bert_gemm_ln_w_supported(Hi, Ii)) {
        for (Layer& l : layers_) {
            BERT_TRY(pack_weights(l.qkv_wp, l.qkv_w, 3 * Hi, Hi));
            BERT_TRY(pack_weights(l.ao_wp, l.ao_w, Hi, Hi));
            BERT_TRY(pack_weights(l.i_wp, l.i_w, Ii, Hi));
            BERT_TRY(pack_weights(l.o_wp, l.o_w, Hi, Ii));
        }
        BERT_HIP(hipDeviceSynchronize());
        packed_ = true;
        if (bert_docs_w_supported(Hi, Ii, (int)cfg.heads)) {
            // the one-launch forward of short texts (bert_docs_w.hip) walks a device table of the layers' pointers
            std::vector<BertDocsLayer> table;
            for (Layer& l : layers_) {
                BertDocsLayer t{};
                t.qkv_wp = l.qkv_wp.ptr;
                t.ao_wp = l.ao_wp.ptr;
                t.i_wp = l.i_wp.ptr;
                t.o_wp = l.o_wp.ptr;
                t.qkv_b = static_cast<const float*>(l.qkv_b.ptr);
                t.ao_b = static_cast<const float*>(l.ao_b.ptr);
                t.ln1_w = static_cast<const float*>(l.ln1_w.ptr);
                t.ln1_b = static_cast<const float*>(l.ln1_b.ptr);
                t.i_b = static_cast<const float*>(l.i_b.ptr);
                t.o_b = static_cast<const float*>(l.o_b.ptr);
                t.ln2_w = static_cast<const float*>(l.ln2_w.ptr);
                t.ln2_b = static_cast<const float*>(l.ln2_b.ptr);
                table.push_back(t);
            }
            BERT_TRY(docs_layers_.reserve(table.size() * sizeof(BertDocsLayer)));
            BERT_HIP(hipMemcpy(docs_layers_.ptr, table.data(), table.size() * sizeof(BertDocsLayer), hipMemcpyHostToDevice));
            docs_ready_ = true;
        }
    }
    return SearchError{};
}

void NativeEmbedder::drop_graphs() {
    for (auto& kv : graphs_)
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
    graphs_.clear();
}

// Workspaces for `tokens` tokens.  Calls that may be graph-captured share buffers sized for kGraphMaxTokens, so a captured
// graph's pointers stay valid; a larger call that has to move a buffer drops the graphs.
SearchError NativeEmbedder::reserve_workspaces(uint32_t tokens) {
    const size_t H = cfg_.hidden, I = cfg_.inter;
    const size_t T = tokens <= kGraphMaxTokens ? kGraphMaxTokens : tokens;
    if (int8_) {   // (int8 mode: no f16 activations but the attention's context)
        const void* before[] = {x_f32_.ptr, qkv_f32_.ptr, ctx_h_.ptr, tmp_f32_.ptr, qx_.ptr, sx_.ptr, inter_f32_.ptr};
        BERT_TRY(x_f32_.reserve(T * H * 4));
        BERT_TRY(qkv_f32_.reserve(T * 3 * H * 4));
        BERT_TRY(ctx_h_.reserve(T * H * 2));
        BERT_TRY(tmp_f32_.reserve(T * H * 4));
        BERT_TRY(qx_.reserve(T * (H > I ? H : I)));
        BERT_TRY(sx_.reserve(T * 4));
        BERT_TRY(inter_f32_.reserve(T * I * 4));
        const void* after[] = {x_f32_.ptr, qkv_f32_.ptr, ctx_h_.ptr, tmp_f32_.ptr, qx_.ptr, sx_.ptr, inter_f32_.ptr};
        for (int i = 0; i < 7; ++i)
            if (before[i] && before[i] != after[i]) {
                drop_graphs();
                break;
            }
        return SearchError{};
    }
    const void* before[] = {x_f32_.ptr, x_h_.ptr, qkv_f32_.ptr, ctx_h_.ptr, tmp_f32_.ptr, inter_h_.ptr};
    BERT_TRY(x_f32_.reserve(T * H * 4));
    BERT_TRY(x_h_.reserve(T * H * 2));
    BERT_TRY(qkv_f32_.reserve(T * 3 * H * 4));
    BERT_TRY(ctx_h_.reserve(T * H * 2));
    BERT_TRY(tmp_f32_.reserve(T * H * 4));
    BERT_TRY(inter_h_.reserve(T * I * 2));
    const void* after[] = {x_f32_.ptr, x_h_.ptr, qkv_f32_.ptr, ctx_h_.ptr, tmp_f32_.ptr, inter_h_.ptr};
    for (int i = 0; i < 6; ++i)
        if (before[i] && before[i] != after[i]) {
            drop_graphs();
            break;
        }
    return SearchError{};
}

bool NativeEmbedder::query_path(uint32_t tokens) const {
    static const bool off = fsgpu::lab_env("FSGPU_BERT_NO_QUERY_PATH") != nullptr;  // A/B runs
    return !off && !int8_ && tokens <= 32 && bert_query_path_supported((int)cfg_.hidden, (int)cfg_.inter, (int)cfg_.heads);
}

bool NativeEmbedder::one_launch_path() const {
    // (measured slower than the replayed graph of 25 launches — bert_query_kernels.hip —: opt-in, experiments builds only)
    static const bool on = fsgpu::lab_env("FSGPU_BERT_ONE_LAUNCH") != nullptr;
    return on && !int8_ && q_one_launch_ok_ && bert_q_one_launch_blocks() > 0;
}

// Query-sized inputs (<= 32 tokens in total): the 25 stages of bert_query_kernels.hip as 4 launches per layer + the pooling (replayed
// from a captured graph by embed_batch) — or, in experiments builds, in ONE launch of 24 resident blocks with grid-wide barriers
// between the stages (slower: see the kernel).
SearchError NativeEmbedder::forward_query(uint32_t n_docs, uint32_t tokens) {
    const int H = (int)cfg_.hidden, I = (int)cfg_.inter;
    BERT_TRY(q_x_.reserve((size_t)2 * 32 * H * 4));
    BERT_TRY(q_parts_.reserve((size_t)4 * 32 * H * 4));
    float* X[2] = {static_cast<float*>(q_x_.ptr), static_cast<float*>(q_x_.ptr) + 32 * H};
    float* parts = static_cast<float*>(q_parts_.ptr);
    const bool one = one_launch_path();
    const uint32_t* offsets = q_offsets_ ? q_offsets_ : static_cast<const uint32_t*>(offsets_.ptr);
    const int32_t* ids = q_ids_ ? q_ids_ : static_cast<const int32_t*>(ids_.ptr);
    const int32_t* positions = q_positions_ ? q_positions_ : static_cast<const int32_t*>(positions_.ptr);
    float* pooled = pooled_out_ ? pooled_out_ : static_cast<float*>(out_.ptr);
    BertQueryArgs base{};
    if (!one) {   // (the one-launch form passes the per-call fields in its own argument block: its stage table does not depend on them)
        base.tokens = (int)tokens;
        base.n_docs = (int)n_docs;
        base.offsets = offsets;
    }
    base.eps = cfg_.ln_eps;
    base.attn_scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    std::vector<BertQueryArgs>& st = q_stages_host_[q_stages_flip_ ^ 1];
    std::vector<unsigned char>& kinds = q_kinds_host_[q_stages_flip_ ^ 1];
    st.clear();
    kinds.clear();
    const Layer* prev = nullptr;
    for (Layer& l : layers_) {
        BertQueryArgs k1 = base;   // [pending LN2 | embedding LN] -> QKV of each head -> attention -> ctx
        if (!prev) {
            k1.ids = one ? static_cast<const int32_t*>(ids_.ptr) : ids;   // (one launch: "non-null" marks the embedding stage)
            k1.positions = one ? nullptr : positions;
            k1.word = static_cast<const float*>(word_.ptr);
            k1.pos = static_cast<const float*>(pos_.ptr);
            k1.type0 = static_cast<const float*>(type_.ptr);
            k1.lnw = static_cast<const float*>(emb_ln_w_.ptr);
            k1.lnb = static_cast<const float*>(emb_ln_b_.ptr);
        } else {
            k1.x_in = X[1];
            k1.parts = parts;
            k1.n_parts = 4;
            k1.prev_bias = static_cast<const float*>(prev->o_b.ptr);
            k1.lnw = static_cast<const float*>(prev->ln2_w.ptr);
            k1.lnb = static_cast<const float*>(prev->ln2_b.ptr);
        }
        k1.x_out = X[0];
        k1.w = static_cast<const _Float16*>(l.qkv_w.ptr);
        k1.ldw = H;
        k1.bias = static_cast<const float*>(l.qkv_b.ptr);
        k1.out_h = static_cast<_Float16*>(ctx_h_.ptr);
        st.push_back(k1);
        kinds.push_back(0);
        BertQueryArgs k2 = base;   // out-projection -> one partial slab
        k2.a_h = static_cast<const _Float16*>(ctx_h_.ptr);
        k2.lda = H;
        k2.w = static_cast<const _Float16*>(l.ao_w.ptr);
        k2.ldw = H;
        k2.n = H;
        k2.out_f32 = parts;
        st.push_back(k2);
        kinds.push_back(1);
        BertQueryArgs k3 = base;   // x = LN1(x + slab + bias) -> FFN-up + GELU
        k3.x_in = X[0];
        k3.x_out = X[1];
        k3.parts = parts;
        k3.n_parts = 1;
        k3.prev_bias = static_cast<const float*>(l.ao_b.ptr);
        k3.lnw = static_cast<const float*>(l.ln1_w.ptr);
        k3.lnb = static_cast<const float*>(l.ln1_b.ptr);
        k3.w = static_cast<const _Float16*>(l.i_w.ptr);
        k3.ldw = H;
        k3.n = I;
        k3.bias = static_cast<const float*>(l.i_b.ptr);
        k3.out_h = static_cast<_Float16*>(inter_h_.ptr);
        st.push_back(k3);
        kinds.push_back(2);
        BertQueryArgs k4 = base;   // FFN-down, K split 4 ways -> four partial slabs
        k4.a_h = static_cast<const _Float16*>(inter_h_.ptr);
        k4.lda = I;
        k4.w = static_cast<const _Float16*>(l.o_w.ptr);
        k4.ldw = I;
        k4.n = H;
        k4.out_f32 = parts;
        st.push_back(k4);
        kinds.push_back(3);
        prev = &l;
    }
    BertQueryArgs kp = base;       // x = LN2(x + slabs + bias) -> mean per text -> L2
    kp.x_in = X[1];
    kp.parts = parts;
    kp.n_parts = 4;
    kp.prev_bias = static_cast<const float*>(prev->o_b.ptr);
    kp.lnw = static_cast<const float*>(prev->ln2_w.ptr);
    kp.lnb = static_cast<const float*>(prev->ln2_b.ptr);
    st.push_back(kp);
    kinds.push_back(4);
    if (!one) {
        for (size_t i = 0; i < st.size(); ++i) {
            if (kinds[i] == 0) BERT_HIP(launch_bert_q_qkv_attn(st[i], (int)cfg_.heads, stream_));
            else if (kinds[i] == 4) BERT_HIP(launch_bert_q_pool(st[i], pooled, stream_));
            else BERT_HIP(launch_bert_q_gemm(st[i], (int)kinds[i] - 1, stream_));
        }
        return SearchError{};
    }
    // the stage table lives on the device; it is sent again only when a pointer in it has changed (a workspace moved)
    const std::vector<BertQueryArgs>& sent = q_stages_host_[q_stages_flip_];
    const size_t table_bytes = st.size() * sizeof(BertQueryArgs);
    if (!q_status_) {
        BERT_HIP(hipHostMalloc(reinterpret_cast<void**>(&q_status_), 64, hipHostMallocMapped));
        *q_status_ = 0;
        BERT_TRY(q_counter_.reserve(64));
        BERT_HIP(hipMemsetAsync(q_counter_.ptr, 0, 64, stream_));
        q_launches_ = 0;
    }
    if (sent.size() != st.size() || std::memcmp(sent.data(), st.data(), table_bytes) != 0 || !q_stages_.ptr) {
        BERT_HIP(hipStreamSynchronize(stream_));   // (rare: nothing may still be reading the old table — or the host copy that fed it)
        BERT_TRY(q_stages_.reserve(table_bytes + 256));
        BERT_HIP(hipMemcpyAsync(q_stages_.ptr, st.data(), table_bytes, hipMemcpyHostToDevice, stream_));
        BERT_HIP(hipMemcpyAsync(static_cast<char*>(q_stages_.ptr) + table_bytes, kinds.data(), kinds.size(), hipMemcpyHostToDevice, stream_));
        BERT_HIP(hipStreamSynchronize(stream_));
        q_stages_flip_ ^= 1;
    }
    const unsigned int barriers = (unsigned int)(st.size() - 1) * (unsigned int)bert_q_one_launch_blocks();
    BERT_HIP(launch_bert_q_one_launch(static_cast<const BertQueryArgs*>(q_stages_.ptr),
                                      static_cast<const unsigned char*>(q_stages_.ptr) + table_bytes, (int)st.size(), (int)tokens, (int)n_docs,
                                      offsets, ids, positions, pooled, static_cast<unsigned int*>(q_counter_.ptr), q_launches_ * barriers,
                                      q_status_, stream_));
    ++q_launches_;
    return SearchError{};
}

SearchError NativeEmbedder::forward_packed_range(uint32_t d0, uint32_t d1, uint32_t t0, uint32_t t1, uint32_t max_seq,
                                                 hipStream_t stream) {
    const int H = (int)cfg_.hidden, I = (int)cfg_.inter, T = (int)(t1 - t0);
    const float eps = cfg_.ln_eps;
    if (T <= 0 || d1 <= d0) return SearchError{};
    float* xa = static_cast<float*>(x_f32_.ptr);                       // whole buffers: attention and pooling index tokens absolutely
    _Float16* xh = static_cast<_Float16*>(x_h_.ptr);
    _Float16* qkv = static_cast<_Float16*>(qkv_f32_.ptr);              // f16 Q, K, V in the first half of the f32 workspace
    _Float16* ctx = static_cast<_Float16*>(ctx_h_.ptr);
    float* x = xa + (size_t)t0 * H;
    _Float16* x_h = xh + (size_t)t0 * H;
    const uint32_t* offs = static_cast<const uint32_t*>(offsets_.ptr) + d0;
    BERT_HIP(launch_bert_embed_ln(static_cast<const int32_t*>(ids_.ptr) + t0, static_cast<const int32_t*>(positions_.ptr) + t0,
                                  static_cast<const float*>(word_.ptr), static_cast<const float*>(pos_.ptr),
                                  static_cast<const float*>(type_.ptr), static_cast<const float*>(emb_ln_w_.ptr),
                                  static_cast<const float*>(emb_ln_b_.ptr), x, x_h, T, H, eps, stream));
    const float scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    for (Layer& l : layers_) {
        BERT_TRY(packed_qkv(l, x_h, qkv + (size_t)t0 * 3 * H, T, false, stream));
        BERT_HIP(launch_bert_attention_h(qkv, offs, ctx, (int)(d1 - d0), (int)cfg_.heads, H, (int)max_seq, scale, stream));
        if (T >= FSGPU_BERT_SPLIT_MIN_TOKENS && bert_gemm_ln_w_supported(H, H) && bert_gemm_ln_w_supported(H, I) && bert_gemm_w_supported(I, H)) {
            // Thousands of rows (the documents of an index build): the one-launch post-attention block re-streams its 2.65 MB of
            // weights for every 32 rows (1.36 GB out of the L2s per layer at 16k tokens: that IS its 90 us).  Here the FFN-up
            // projection is the weight-stationary GEMM (bert_gemm_wp_kernel: a block keeps its weight slice in registers and
            // walks the row tiles), its 16-bit activations go through L2 / the Infinity Cache, and the two LayerNorm projections
            // stream their weights once per 32-row block.
            _Float16* inter = static_cast<_Float16*>(inter_h_.ptr) + (size_t)t0 * I;
            BERT_HIP(launch_bert_gemm_ln_w(ctx + (size_t)t0 * H, l.ao_wp.ptr, static_cast<const float*>(l.ao_b.ptr), x, x_h,
                                           static_cast<const float*>(l.ln1_w.ptr), static_cast<const float*>(l.ln1_b.ptr), T, H, H, eps, stream));
            BERT_HIP(launch_bert_gemm_w(x_h, l.i_wp.ptr, static_cast<const float*>(l.i_b.ptr), nullptr, inter, T, I, H, 1, stream));
            BERT_HIP(launch_bert_gemm_ln_w(inter, l.o_wp.ptr, static_cast<const float*>(l.o_b.ptr), x, x_h,
                                           static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr), T, H, I, eps, stream));
            continue;
        }
        BERT_TRY(packed_post_attention(l, ctx + (size_t)t0 * H, x, x_h, T, false, stream));
    }
    float* out = (pooled_out_ ? pooled_out_ : static_cast<float*>(out_.ptr)) + (size_t)d0 * H;
    BERT_HIP(launch_bert_pool(xa, offs, out, (int)(d1 - d0), H, stream));
    return SearchError{};
}

SearchError NativeEmbedder::packed_qkv(const Layer& l, const _Float16* x_h, _Float16* qkv, int T, bool fixed, hipStream_t stream) {
    const int H = (int)cfg_.hidden;
    const float* bias = static_cast<const float*>(l.qkv_b.ptr);
    if (fixed) BERT_HIP(launch_bert_gemm_w_fixed(x_h, l.qkv_wp.ptr, bias, nullptr, qkv, T, 3 * H, H, 2, stream));
    else BERT_HIP(launch_bert_gemm_w(x_h, l.qkv_wp.ptr, bias, nullptr, qkv, T, 3 * H, H, 2, stream));
    return SearchError{};
}

SearchError NativeEmbedder::packed_post_attention(const Layer& l, const _Float16* ctx, float* x, _Float16* x_h, int M, bool fixed,
                                                  hipStream_t stream) {
    const int H = (int)cfg_.hidden, I = (int)cfg_.inter;
    auto launch = fixed ? launch_bert_post_attn_w_fixed : launch_bert_post_attn_w;
    BERT_HIP(launch(ctx, l.ao_wp.ptr, static_cast<const float*>(l.ao_b.ptr), static_cast<const float*>(l.ln1_w.ptr),
                    static_cast<const float*>(l.ln1_b.ptr), l.i_wp.ptr, static_cast<const float*>(l.i_b.ptr), l.o_wp.ptr,
                    static_cast<const float*>(l.o_b.ptr), x, x_h, static_cast<const float*>(l.ln2_w.ptr),
                    static_cast<const float*>(l.ln2_b.ptr), M, H, I, cfg_.ln_eps, stream));
    return SearchError{};
}

// int8 mode: every batch shape takes this chain.  Per layer: QKV (one [3H, H] int8 linear) -> the f32-operand attention
// (bert_kernels.hip) -> quantise the f16 context -> AO -> add + LN + quantise -> FFN-in + GELU -> quantise -> FFN-out -> add + LN
// (+ quantise for the next layer).  Every kernel of it computes a row (a text, for the attention and the pooling) from that row alone.
SearchError NativeEmbedder::forward_int8(uint32_t n_docs, uint32_t tokens, uint32_t max_seq) {
    const int H = (int)cfg_.hidden, I = (int)cfg_.inter, T = (int)tokens;
    const float eps = cfg_.ln_eps;
    float* x = static_cast<float*>(x_f32_.ptr);
    float* qkv = static_cast<float*>(qkv_f32_.ptr);
    float* tmp = static_cast<float*>(tmp_f32_.ptr);
    float* inter = static_cast<float*>(inter_f32_.ptr);
    float* sx = static_cast<float*>(sx_.ptr);
    void* qx = qx_.ptr;
    const uint32_t* offs = static_cast<const uint32_t*>(offsets_.ptr);
    BERT_HIP(launch_bert_i8_embed_ln_quant(static_cast<const int32_t*>(ids_.ptr), static_cast<const int32_t*>(positions_.ptr),
                                           static_cast<const float*>(word_.ptr), static_cast<const float*>(pos_.ptr),
                                           static_cast<const float*>(type_.ptr), static_cast<const float*>(emb_ln_w_.ptr),
                                           static_cast<const float*>(emb_ln_b_.ptr), x, qx, sx, T, H, eps, stream_));
    const float scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    for (size_t li = 0; li < layers_.size(); ++li) {
        Layer& l = layers_[li];
        const bool last = li + 1 == layers_.size();
        BERT_HIP(launch_bert_i8_gemm(qx, sx, l.qkv_q.ptr, static_cast<const float*>(l.qkv_s.ptr), static_cast<const float*>(l.qkv_b.ptr),
                                     qkv, T, 3 * H, H, false, stream_));
        BERT_HIP(launch_bert_attention(qkv, offs, ctx_h_.ptr, (int)n_docs, (int)cfg_.heads, H, (int)max_seq, scale, stream_));
        BERT_HIP(launch_bert_i8_quant_rows_h(ctx_h_.ptr, qx, sx, T, H, stream_));
        BERT_HIP(launch_bert_i8_gemm(qx, sx, l.ao_q.ptr, static_cast<const float*>(l.ao_s.ptr), static_cast<const float*>(l.ao_b.ptr), tmp,
                                     T, H, H, false, stream_));
        BERT_HIP(launch_bert_i8_add_ln_quant(x, tmp, static_cast<const float*>(l.ln1_w.ptr), static_cast<const float*>(l.ln1_b.ptr), qx, sx,
                                             T, H, eps, stream_));
        BERT_HIP(launch_bert_i8_gemm(qx, sx, l.i_q.ptr, static_cast<const float*>(l.i_s.ptr), static_cast<const float*>(l.i_b.ptr), inter,
                                     T, I, H, true, stream_));
        BERT_HIP(launch_bert_i8_quant_rows(inter, qx, sx, T, I, stream_));
        BERT_HIP(launch_bert_i8_gemm(qx, sx, l.o_q.ptr, static_cast<const float*>(l.o_s.ptr), static_cast<const float*>(l.o_b.ptr), tmp,
                                     T, H, I, false, stream_));
        BERT_HIP(launch_bert_i8_add_ln_quant(x, tmp, static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr),
                                             last ? nullptr : qx, sx, T, H, eps, stream_));
    }
    BERT_HIP(launch_bert_pool(x, offs, pooled_out_ ? pooled_out_ : static_cast<float*>(out_.ptr), (int)n_docs, H, stream_));
    return SearchError{};
}

SearchError NativeEmbedder::forward(uint32_t n_docs, uint32_t tokens, uint32_t max_seq) {
    const int H = (int)cfg_.hidden, I = (int)cfg_.inter, T = (int)tokens;
    const float eps = cfg_.ln_eps;
    if (int8_) return forward_int8(n_docs, tokens, max_seq);
    if (query_path(tokens)) return forward_query(n_docs, tokens);
    {
        static const bool ab = fsgpu::lab_env("FSGPU_BERT_SPLIT_AO") || fsgpu::lab_env("FSGPU_BERT_SPLIT_FFN");   // A/B runs below
        static const int packed_min0 = [] {
            const char* e = fsgpu::lab_env("FSGPU_BERT_PACKED_MIN_TOKENS");
            return e ? std::atoi(e) : 32;
        }();
        if (packed_ && !ab && (int)tokens > packed_min0 && bert_post_attn_w_supported((int)cfg_.hidden, (int)cfg_.inter)) {
            // (the batch as two halves on two streams — most kernels fill only part of the chip — was tried: the branches of
            // the replayed graph did not overlap and 256 queries went from 0.43 to 0.50 ms)
            return forward_packed_range(0, n_docs, 0, tokens, max_seq, stream_);
        }
    }
    float* x = static_cast<float*>(x_f32_.ptr);
    float* tmp = static_cast<float*>(tmp_f32_.ptr);
    float* qkv = static_cast<float*>(qkv_f32_.ptr);
    const uint32_t* offs = static_cast<const uint32_t*>(offsets_.ptr);
    BERT_HIP(launch_bert_embed_ln(static_cast<const int32_t*>(ids_.ptr), static_cast<const int32_t*>(positions_.ptr),
                                  static_cast<const float*>(word_.ptr), static_cast<const float*>(pos_.ptr),
                                  static_cast<const float*>(type_.ptr), static_cast<const float*>(emb_ln_w_.ptr),
                                  static_cast<const float*>(emb_ln_b_.ptr), x, x_h_.ptr, T, H, eps, stream_));
    const float scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    static const bool no_fuse = fsgpu::lab_env("FSGPU_BERT_NO_FUSED_LN") != nullptr;  // A/B runs
    // a batch fills the chip with 32-row blocks; a single query (a few tokens) would run each projection on ONE block
    // and is quicker through the 32x64-tile GEMM + the stand-alone add+LN kernel (measured 0.36 vs 0.43 ms)
    const bool fused_ln = !no_fuse && T > 256 && bert_gemm_ln_supported(H) && (H % 32 == 0) && (I % 32 == 0);
    // a batch: every linear over the fragment-order weights (bert_gemm_w.hip) — 3 launches per layer (QKV, attention, the rest)
    static const int packed_min = [] {
        // above the query path's 32 tokens every size is quicker here (2 queries 0.37 -> 0.30 ms, 12 queries 0.47 -> 0.32 ms)
        const char* e = fsgpu::lab_env("FSGPU_BERT_PACKED_MIN_TOKENS");   // tuning runs
        return e ? std::atoi(e) : 32;
    }();
    const bool packed = packed_ && T > packed_min;
    for (Layer& l : layers_) {
        if (packed) {
            // Q, K, V leave the projection as f16 (what the attention's matrix-core operands are rounded to anyway) in the
            // first half of the f32 QKV workspace
            BERT_HIP(launch_bert_gemm_w(x_h_.ptr, l.qkv_wp.ptr, static_cast<const float*>(l.qkv_b.ptr), nullptr, qkv, T, 3 * H, H,
                                        2, stream_));
            BERT_HIP(launch_bert_attention_h(qkv, offs, ctx_h_.ptr, (int)n_docs, (int)cfg_.heads, H, (int)max_seq, scale,
                                             stream_));
            static const bool split_ao = fsgpu::lab_env("FSGPU_BERT_SPLIT_AO") != nullptr;     // A/B runs: output projection apart
            static const bool split_ffn0 = fsgpu::lab_env("FSGPU_BERT_SPLIT_FFN") != nullptr;
            if (!split_ao && !split_ffn0 && bert_post_attn_w_supported(H, I)) {
                BERT_HIP(launch_bert_post_attn_w(ctx_h_.ptr, l.ao_wp.ptr, static_cast<const float*>(l.ao_b.ptr),
                                                 static_cast<const float*>(l.ln1_w.ptr), static_cast<const float*>(l.ln1_b.ptr),
                                                 l.i_wp.ptr, static_cast<const float*>(l.i_b.ptr), l.o_wp.ptr,
                                                 static_cast<const float*>(l.o_b.ptr), x, x_h_.ptr,
                                                 static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr), T, H,
                                                 I, eps, stream_));
                continue;
            }
            BERT_HIP(launch_bert_gemm_ln_w(ctx_h_.ptr, l.ao_wp.ptr, static_cast<const float*>(l.ao_b.ptr), x, x_h_.ptr,
                                           static_cast<const float*>(l.ln1_w.ptr), static_cast<const float*>(l.ln1_b.ptr), T, H,
                                           H, eps, stream_));
            static const bool split_ffn = fsgpu::lab_env("FSGPU_BERT_SPLIT_FFN") != nullptr;   // A/B runs: two launches
            if (!split_ffn && bert_ffn_w_supported(H, I)) {
                BERT_HIP(launch_bert_ffn_w(l.i_wp.ptr, static_cast<const float*>(l.i_b.ptr), l.o_wp.ptr,
                                           static_cast<const float*>(l.o_b.ptr), x, x_h_.ptr,
                                           static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr), T, H,
                                           I, eps, stream_));
                continue;
            }
            BERT_HIP(launch_bert_gemm_w(x_h_.ptr, l.i_wp.ptr, static_cast<const float*>(l.i_b.ptr), nullptr, inter_h_.ptr, T, I,
                                        H, 1, stream_));
            BERT_HIP(launch_bert_gemm_ln_w(inter_h_.ptr, l.o_wp.ptr, static_cast<const float*>(l.o_b.ptr), x, x_h_.ptr,
                                           static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr), T, H,
                                           I, eps, stream_));
            continue;
        }
        BERT_HIP(launch_bert_gemm(x_h_.ptr, l.qkv_w.ptr, static_cast<const float*>(l.qkv_b.ptr), qkv, nullptr, T, 3 * H, H,
                                  false, stream_));
        BERT_HIP(launch_bert_attention(qkv, offs, ctx_h_.ptr, (int)n_docs, (int)cfg_.heads, H, (int)max_seq, scale,
                                       stream_));
        if (fused_ln) {
            BERT_HIP(launch_bert_gemm_ln(ctx_h_.ptr, l.ao_w.ptr, static_cast<const float*>(l.ao_b.ptr), x, x_h_.ptr,
                                         static_cast<const float*>(l.ln1_w.ptr), static_cast<const float*>(l.ln1_b.ptr), T, H,
                                         H, eps, stream_));
        } else {
            BERT_HIP(launch_bert_gemm(ctx_h_.ptr, l.ao_w.ptr, static_cast<const float*>(l.ao_b.ptr), tmp, nullptr, T, H, H,
                                      false, stream_));
            BERT_HIP(launch_bert_add_ln(x, tmp, static_cast<const float*>(l.ln1_w.ptr),
                                        static_cast<const float*>(l.ln1_b.ptr), x_h_.ptr, T, H, eps, stream_));
        }
        BERT_HIP(launch_bert_gemm(x_h_.ptr, l.i_w.ptr, static_cast<const float*>(l.i_b.ptr), nullptr, inter_h_.ptr, T, I, H,
                                  true, stream_));
        if (fused_ln) {
            BERT_HIP(launch_bert_gemm_ln(inter_h_.ptr, l.o_w.ptr, static_cast<const float*>(l.o_b.ptr), x, x_h_.ptr,
                                         static_cast<const float*>(l.ln2_w.ptr), static_cast<const float*>(l.ln2_b.ptr), T, H,
                                         I, eps, stream_));
        } else {
            BERT_HIP(launch_bert_gemm(inter_h_.ptr, l.o_w.ptr, static_cast<const float*>(l.o_b.ptr), tmp, nullptr, T, H, I,
                                      false, stream_));
            BERT_HIP(launch_bert_add_ln(x, tmp, static_cast<const float*>(l.ln2_w.ptr),
                                        static_cast<const float*>(l.ln2_b.ptr), x_h_.ptr, T, H, eps, stream_));
        }
    }
    BERT_HIP(launch_bert_pool(x, offs, pooled_out_ ? pooled_out_ : static_cast<float*>(out_.ptr), (int)n_docs, H, stream_));
    return SearchError{};
}

bool NativeEmbedder::docs_path(uint32_t tokens, uint32_t max_seq) const {
    static const bool off = fsgpu::lab_env("FSGPU_BERT_NO_DOCS_PATH") != nullptr;  // A/B runs
    // (lab: above this many tokens a batch of short texts takes the three-launches-per-layer path instead — measured the same from
    // 768 texts on and slower below: scripts/r06/exp_enc_paths.py)
    static const long max_tokens = [] {
        const char* e = fsgpu::lab_env("FSGPU_BERT_DOCS_MAX_TOKENS");
        return e ? std::atol(e) : (1L << 30);
    }();
    return !off && !int8_ && docs_ready_ && tokens > 32 && max_seq <= 32 && (long)tokens <= max_tokens;
}

// Consecutive texts are packed greedily into row blocks of at most 32 tokens; a block never splits a text.
BertDocsPacking bert_docs_pack(const int32_t* ids, const uint32_t* offs, uint32_t n, uint32_t total) {
    BertDocsPacking p;
    p.n = n;
    std::vector<uint32_t>& blk_tok = p.blk_tok;
    std::vector<uint32_t>& blk_doc = p.blk_doc;
    blk_tok.reserve(n + 1);
    blk_doc.reserve(n + 1);
    blk_tok.push_back(0);
    blk_doc.push_back(0);
    uint32_t rows = 0;
    for (uint32_t i = 0; i < n; ++i) {
        const uint32_t len = offs[i + 1] - offs[i];
        if (rows + len > 32) {   // (rows > 0 here: len <= 32)
            blk_tok.push_back(offs[i]);
            blk_doc.push_back(i);
            rows = 0;
        }
        rows += len;
    }
    blk_tok.push_back(total);
    blk_doc.push_back(n);
    const uint32_t nblocks = (uint32_t)blk_tok.size() - 1;
    p.nblocks = nblocks;
    // the blocks' rows, laid out so that a block needs ONE read of the inputs before its embedding gather: token id (-1 = padding),
    // rows of the block << 16 | position inside the text << 8 | the text's index among the block's non-empty texts
    p.row_id.assign((size_t)nblocks * 32, -1);
    p.row_meta.assign((size_t)nblocks * 32, 0u);
    std::vector<int32_t>& row_id = p.row_id;
    std::vector<uint32_t>& row_meta = p.row_meta;
    for (uint32_t b = 0; b < nblocks; ++b) {
        const uint32_t t0 = blk_tok[b], nrows = blk_tok[b + 1] - t0;
        uint32_t local = 0;
        for (uint32_t r = 0; r < 32; ++r) row_meta[(size_t)b * 32 + r] = nrows << 16;
        for (uint32_t i = blk_doc[b]; i < blk_doc[b + 1]; ++i) {
            if (offs[i + 1] == offs[i]) continue;
            for (uint32_t t = offs[i]; t < offs[i + 1]; ++t) {
                if (ids) row_id[(size_t)b * 32 + (t - t0)] = ids[t];
                row_meta[(size_t)b * 32 + (t - t0)] |= ((t - offs[i]) << 8) | local;
            }
            ++local;
        }
    }
    // one input block: [offsets | blk_tok | blk_doc | row_id | row_meta]
    p.o_tok = (size_t)(n + 1) * 4;
    p.o_doc = p.o_tok + (size_t)(nblocks + 1) * 4;
    p.o_rid = p.o_doc + (size_t)(nblocks + 1) * 4;
    p.o_rmeta = p.o_rid + (size_t)nblocks * 32 * 4;
    p.in_bytes = (p.o_rmeta + (size_t)nblocks * 32 * 4 + 255) & ~(size_t)255;
    return p;
}

void BertDocsPacking::fill(unsigned char* dst, const uint32_t* offs) const {
    std::memcpy(dst, offs, (size_t)(n + 1) * 4);
    std::memcpy(dst + o_tok, blk_tok.data(), (size_t)(nblocks + 1) * 4);
    std::memcpy(dst + o_doc, blk_doc.data(), (size_t)(nblocks + 1) * 4);
    std::memcpy(dst + o_rid, row_id.data(), row_id.size() * 4);
    std::memcpy(dst + o_rmeta, row_meta.data(), row_meta.size() * 4);
}

void BertDocsPacking::point(BertDocsArgs& a, const unsigned char* base) const {
    a.offsets = reinterpret_cast<const uint32_t*>(base);
    a.blk_tok = reinterpret_cast<const uint32_t*>(base + o_tok);
    a.blk_doc = reinterpret_cast<const uint32_t*>(base + o_doc);
    a.row_id = reinterpret_cast<const int32_t*>(base + o_rid);
    a.row_meta = reinterpret_cast<const uint32_t*>(base + o_rmeta);
}

// Every text at most 32 tokens long (a batch of queries): ONE launch for the whole forward (bert_docs_w.hip) over the row blocks of
// bert_docs_pack.  ids: this call's tokens; offs: the call's offsets rebased to 0.
SearchError NativeEmbedder::embed_docs(const int32_t* ids, const std::vector<uint32_t>& offs, uint32_t n, uint32_t total, float* out,
                                       float* out_dev, bool ids_on_device) {
    const size_t H = cfg_.hidden;
    const BertDocsPacking pk = bert_docs_pack(ids_on_device ? nullptr : ids, offs.data(), n, total);
    const uint32_t nblocks = pk.nblocks;
    const size_t in_bytes = pk.in_bytes;
    const size_t out_bytes = (size_t)n * H * 4;
    const bool pinned = !ids_on_device && in_bytes + out_bytes <= kDocsIoBytes;   // (device ids stay on the device)
    if (pinned && !docs_io_ && !docs_io_failed_ && hipHostMalloc(&docs_io_, kDocsIoBytes, hipHostMallocMapped) != hipSuccess) {
        docs_io_ = nullptr;
        docs_io_failed_ = true;
        (void)hipGetLastError();
    }
    BertDocsArgs a{};
    a.word = static_cast<const float*>(word_.ptr);
    a.pos = static_cast<const float*>(pos_.ptr);
    a.type0 = static_cast<const float*>(type_.ptr);
    a.emb_lnw = static_cast<const float*>(emb_ln_w_.ptr);
    a.emb_lnb = static_cast<const float*>(emb_ln_b_.ptr);
    a.layers = static_cast<const BertDocsLayer*>(docs_layers_.ptr);
    a.nlayers = (int)cfg_.layers;
    a.eps = cfg_.ln_eps;
    a.attn_scale = 0.17677669f;  // ATTN_SCALE_F32 = 1/sqrt(32) (native.rs:44)
    auto fill = [&](unsigned char* dst) { pk.fill(dst, offs.data()); };
    auto point = [&](const unsigned char* base) { pk.point(a, base); };
    if (pinned && docs_io_) {
        // the blocks read their rows in place from the pinned block (mapped into the device's address
        // space) and the pooled vectors land in it: no copy in either direction
        unsigned char* io = static_cast<unsigned char*>(docs_io_);
        fill(io);
        point(io);
        a.out = out_dev ? out_dev : reinterpret_cast<float*>(io + in_bytes);   // (device output: the pooled vectors stay in HBM)
#ifdef FSGPU_EXPERIMENTS
        static const bool trace = fsgpu::lab_env("FSGPU_BERT_DOCS_STAMPS") != nullptr;   // per-phase shader clocks of block 0
        static unsigned long long* stamps = nullptr;
        if (trace && !stamps) (void)hipHostMalloc(reinterpret_cast<void**>(&stamps), 128 * 8, hipHostMallocMapped);
        if (trace && stamps) {
            std::memset(stamps, 0, 128 * 8);
            a.stamps = stamps;
        }
#endif
        BERT_HIP(launch_bert_docs_w(a, nblocks, stream_));
        BERT_HIP(hipStreamSynchronize(stream_));
#ifdef FSGPU_EXPERIMENTS
        if (a.stamps) {
            std::fprintf(stderr, "[docs stamps]");
            for (int i = 1; i < 4 + 8 * (int)cfg_.layers; ++i)
                std::fprintf(stderr, " %lld", a.stamps[i] ? (long long)(a.stamps[i] - a.stamps[0]) : -1ll);
            std::fprintf(stderr, "\n");
        }
#endif
        if (out_dev && out) BERT_HIP(hipMemcpy(out, out_dev, out_bytes, hipMemcpyDeviceToHost));
        else if (out) std::memcpy(out, io + in_bytes, out_bytes);
        return SearchError{};
    }
    std::vector<unsigned char> host(in_bytes);
    fill(host.data());
    BERT_TRY(docs_in_.reserve(in_bytes));
    BERT_TRY(docs_out_.reserve(out_bytes));   // (not out_: captured graphs name that one)
    BERT_HIP(hipMemcpyAsync(docs_in_.ptr, host.data(), in_bytes, hipMemcpyHostToDevice, stream_));
    point(static_cast<const unsigned char*>(docs_in_.ptr));
    if (ids_on_device)   // the blocks' row ids, from the ids where they lie (the copy above left them at -1)
        BERT_HIP(launch_wordpiece_block_rows(ids, a.blk_tok, reinterpret_cast<int32_t*>(static_cast<unsigned char*>(docs_in_.ptr) + pk.o_rid),
                                             nblocks, stream_));
    a.out = out_dev ? out_dev : static_cast<float*>(docs_out_.ptr);
    BERT_HIP(launch_bert_docs_w(a, nblocks, stream_));
    if (out) BERT_HIP(hipMemcpyAsync(out, a.out, out_bytes, hipMemcpyDeviceToHost, stream_));
    BERT_HIP(hipStreamSynchronize(stream_));
    return SearchError{};
}

SearchError NativeEmbedder::embed_batch(const int32_t* ids, const uint32_t* offsets, uint32_t n, float* out, float* out_dev) {
    return embed_any(ids, false, offsets, n, out, out_dev);
}

SearchError NativeEmbedder::embed_batch_device_ids(const int32_t* ids_dev, const uint32_t* offsets, uint32_t n, float* out, float* out_dev) {
    return embed_any(ids_dev, true, offsets, n, out, out_dev);
}

// ids_on_device: `ids` is device memory and is never read on the host (its range is the caller's word: the tokenizer's vocabulary).
SearchError NativeEmbedder::embed_any(const int32_t* ids, bool ids_on_device, const uint32_t* offsets, uint32_t n, float* out,
                                      float* out_dev) {
    if (n == 0) return SearchError{};
    if (!offsets || (!out && !out_dev)) return err(FSGPU_ERR_NULL_ARGUMENT, "offsets/out is null");
    std::lock_guard<std::mutex> lock(mu_);
    uint32_t max_seq = 0;
    for (uint32_t i = 0; i < n; ++i) {
        if (offsets[i + 1] < offsets[i]) return err(FSGPU_ERR_INVALID_CONFIG, "offsets must be non-decreasing");
        const uint32_t len = offsets[i + 1] - offsets[i];
        if (len > cfg_.max_pos)
            return err(FSGPU_ERR_INVALID_CONFIG, "sequence longer than max_position_embeddings (truncate to 512 first)");
        if (len > max_seq) max_seq = len;
    }
    const uint32_t base = offsets[0];
    const uint32_t total = offsets[n] - base;
    const size_t H = cfg_.hidden;
    if (total == 0) {  // every text empty -> zeros (native.rs:1146-1148)
        if (out) std::fill(out, out + (size_t)n * H, 0.0f);
        if (out_dev) {
            BERT_HIP(hipSetDevice(device_));
            BERT_HIP(hipMemsetAsync(out_dev, 0, (size_t)n * H * 4, stream_));
            BERT_HIP(hipStreamSynchronize(stream_));
        }
        return SearchError{};
    }
    if (!ids) return err(FSGPU_ERR_NULL_ARGUMENT, "ids is null");
    std::vector<int32_t> positions(total);
    std::vector<uint32_t> offs(n + 1);
    for (uint32_t i = 0; i <= n; ++i) offs[i] = offsets[i] - base;
    for (uint32_t i = 0; i < n; ++i)
        for (uint32_t t = offs[i]; t < offs[i + 1]; ++t) {
            if (!ids_on_device) {
                const int32_t id = ids[base + t];
                if (id < 0 || (uint32_t)id >= cfg_.vocab) return err(FSGPU_ERR_INVALID_CONFIG, "token id out of vocabulary");
            }
            positions[t] = (int32_t)(t - offs[i]);  // positions restart at 0 per input (native.rs:1159-1167)
        }
    BERT_HIP(hipSetDevice(device_));
    if (docs_path(total, max_seq)) return embed_docs(ids + base, offs, n, total, out, out_dev, ids_on_device);
    {
        // (graph-eligible calls share buffers of the graph-eligible maximum: see reserve_workspaces)
        const bool small = total <= kGraphMaxTokens;
        const void* before[] = {ids_.ptr, positions_.ptr, offsets_.ptr, out_.ptr};
        BERT_TRY(ids_.reserve((size_t)(small ? kGraphMaxTokens : total) * 4));
        BERT_TRY(positions_.reserve((size_t)(small ? kGraphMaxTokens : total) * 4));
        BERT_TRY(offsets_.reserve((size_t)((small ? kGraphMaxTokens : n) + 1) * 4));
        BERT_TRY(out_.reserve((size_t)(small && n <= kGraphMaxTokens ? kGraphMaxTokens : n) * H * 4));
        const void* after[] = {ids_.ptr, positions_.ptr, offsets_.ptr, out_.ptr};
        for (int i = 0; i < 4; ++i)
            if (before[i] && before[i] != after[i]) {
                drop_graphs();
                break;
            }
    }
    BERT_TRY(reserve_workspaces(total));
    // Small calls (queries): inputs go through one pinned block (DMA instead of the runtime's pageable staging) and the
    // pooled vectors are read back from pinned memory the pool kernel wrote — no D2H copy.
    const size_t in_bytes = ((size_t)total * 8 + (size_t)(n + 1) * 4 + 255) & ~(size_t)255;
    const size_t out_bytes = (size_t)n * H * 4;
    const bool small_io = !ids_on_device && in_bytes + out_bytes <= kPinnedIoBytes;   // (device ids: no pinned block, no graph)
    if (small_io) {
        if (!io_host_ && !io_failed_ && hipHostMalloc(&io_host_, kPinnedIoBytes, hipHostMallocMapped) != hipSuccess) {
            io_host_ = nullptr;
            io_failed_ = true;
            (void)hipGetLastError();
        }
    }
    auto run_once = [&]() -> SearchError {
        if (io_host_ && small_io) {
            unsigned char* io = static_cast<unsigned char*>(io_host_);
            std::memcpy(io, ids + base, (size_t)total * 4);
            std::memcpy(io + (size_t)total * 4, positions.data(), (size_t)total * 4);
            std::memcpy(io + (size_t)total * 8, offs.data(), (size_t)(n + 1) * 4);
            auto enqueue = [&]() -> SearchError {
                const bool direct = query_path(total);
                if (direct) {
                    // a query's few dozen ids are read by the first kernel straight from the pinned block (mapped into the
                    // device's address space): three copy nodes of ~4 us each cost more than the forward's first stage
                    q_ids_ = reinterpret_cast<const int32_t*>(io);
                    q_positions_ = reinterpret_cast<const int32_t*>(io + (size_t)total * 4);
                    q_offsets_ = reinterpret_cast<const uint32_t*>(io + (size_t)total * 8);
                } else {
                    BERT_HIP(hipMemcpyAsync(ids_.ptr, io, (size_t)total * 4, hipMemcpyHostToDevice, stream_));
                    BERT_HIP(hipMemcpyAsync(positions_.ptr, io + (size_t)total * 4, (size_t)total * 4, hipMemcpyHostToDevice, stream_));
                    BERT_HIP(hipMemcpyAsync(offsets_.ptr, io + (size_t)total * 8, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, stream_));
                }
                pooled_out_ = reinterpret_cast<float*>(io + in_bytes);
                SearchError fe = forward(n, total, max_seq);
                pooled_out_ = nullptr;
                q_ids_ = q_positions_ = nullptr;
                q_offsets_ = nullptr;
                return fe;
            };
            static const bool no_graph = std::getenv("FSGPU_BERT_NO_GRAPH") != nullptr;  // A/B runs
            bool replayed = false;
            // (the one-launch query forward is a single kernel whose barrier base changes per call: nothing to replay)
        if (graphs_enabled_ && !no_graph && total <= kGraphMaxTokens && !(query_path(total) && one_launch_path())) {
                const auto key = std::make_tuple(n, total, max_seq);
                auto it = graphs_.find(key);
                if (it == graphs_.end()) {
                    if (graphs_.size() >= kGraphMaxEntries) drop_graphs();
                    it = graphs_.emplace(key, GraphEntry{}).first;
                }
                GraphEntry& ge = it->second;
                ++ge.seen;
                if (!ge.exec && ge.seen >= 2) {
                    // second sighting of this shape (the first ran eagerly, so every one-time kernel attribute is set): capture
                    hipGraph_t graph = nullptr;
                    hipError_t ce = hipStreamBeginCapture(stream_, hipStreamCaptureModeThreadLocal);
                    if (ce == hipSuccess) {
                        SearchError fe = enqueue();
                        ce = hipStreamEndCapture(stream_, &graph);
                        if (fe.ok() && ce == hipSuccess && graph) ce = hipGraphInstantiate(&ge.exec, graph, nullptr, nullptr, 0);
                        else if (ce == hipSuccess) ce = hipErrorUnknown;
                        if (graph) (void)hipGraphDestroy(graph);
                    }
                    if (ce != hipSuccess) {   // capture is an optimisation: fall back to eager launches for good
                        if (std::getenv("FSGPU_DEBUG_GRAPH")) std::fprintf(stderr, "[fsgpu bert] graph capture failed: %s\n", hipGetErrorString(ce));
                        (void)hipGetLastError();
                        if (ge.exec) (void)hipGraphExecDestroy(ge.exec);
                        ge.exec = nullptr;
                        graphs_enabled_ = false;
                    }
                }
                if (ge.exec) {
                    BERT_HIP(hipGraphLaunch(ge.exec, stream_));
                    replayed = true;
                }
            }
            if (!replayed) BERT_TRY(enqueue());
            // (device output of a graph-replayed call: the pool kernel's destination is baked into the graph — the pinned block —, so
            // the few KB go back up from there behind it)
            if (out_dev) BERT_HIP(hipMemcpyAsync(out_dev, io + in_bytes, out_bytes, hipMemcpyHostToDevice, stream_));
            BERT_HIP(hipStreamSynchronize(stream_));
            if (out) std::memcpy(out, io + in_bytes, out_bytes);
            return SearchError{};
        }
        BERT_HIP(hipMemcpyAsync(ids_.ptr, ids + base, (size_t)total * 4, ids_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, stream_));
        BERT_HIP(hipMemcpyAsync(positions_.ptr, positions.data(), (size_t)total * 4, hipMemcpyHostToDevice, stream_));
        BERT_HIP(hipMemcpyAsync(offsets_.ptr, offs.data(), (size_t)(n + 1) * 4, hipMemcpyHostToDevice, stream_));
        pooled_out_ = out_dev;   // (null: the pool kernel writes out_)
        const SearchError fe = forward(n, total, max_seq);
        pooled_out_ = nullptr;
        BERT_TRY(fe);
        if (out) BERT_HIP(hipMemcpyAsync(out, out_dev ? out_dev : out_.ptr, (size_t)n * H * 4, hipMemcpyDeviceToHost, stream_));
        BERT_HIP(hipStreamSynchronize(stream_));
        return SearchError{};

    };
    SearchError re = run_once();
    // (the one-launch query forward gave a grid-wide barrier up: never seen, but a wait that cannot end must not be the alternative —
    // the result is discarded, the 25-launch form answers this call and every later one)
    if (re.ok() && q_status_ && *q_status_ != 0) {
        q_one_launch_ok_ = false;
        *q_status_ = 0;
        re = run_once();
    }
    return re;
}

}  // namespace fsgpu

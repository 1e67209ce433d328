// hash_embedder.cpp — host side of the device HashEmbedder (hash_embedder.hpp).
//
// Restated from crates/frankensearch-embed/src/hash_embedder.rs: HashEmbedder::new :215-223 (dimension 0 panics there, refused
// here), embed_batch_sync :254-260.  Everything a text can be refused for is decided here, before a kernel is launched: the
// offsets, the 32 MiB bound, and that the bytes are what a &str holds (the device then decodes without a second validation,
// only clamping its reads to the text).
#include "hash_embedder.hpp"

#include <string>

#include "../../include/fsgpu.h"
#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

namespace {

// Strict UTF-8 (the Unicode standard's table 3-7, what core::str::from_utf8 accepts).
bool well_formed_utf8(const uint8_t* p, const uint8_t* end) {
    while (p < end) {
        const uint8_t b0 = *p;
        if (b0 < 0x80) {
            ++p;
            continue;
        }
        uint32_t need;
        uint8_t lo = 0x80, hi = 0xbf;   // bounds of the second byte
        if (b0 >= 0xc2 && b0 <= 0xdf) {
            need = 2;
        } else if (b0 >= 0xe0 && b0 <= 0xef) {
            need = 3;
            if (b0 == 0xe0) lo = 0xa0;   // no overlong forms
            if (b0 == 0xed) hi = 0x9f;   // no surrogates
        } else if (b0 >= 0xf0 && b0 <= 0xf4) {
            need = 4;
            if (b0 == 0xf0) lo = 0x90;   // no overlong forms
            if (b0 == 0xf4) hi = 0x8f;   // nothing past U+10FFFF
        } else {
            return false;   // a continuation byte, 0xc0 / 0xc1, 0xf5 and above
        }
        if ((size_t)(end - p) < need) return false;
        if (p[1] < lo || p[1] > hi) return false;
        for (uint32_t i = 2; i < need; ++i)
            if ((p[i] & 0xc0) != 0x80) return false;
        p += need;
    }
    return true;
}

}  // namespace

uint32_t hash_embed_first_bad_text(const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, bool has_bitmap) {
    for (uint32_t i = 0; i < n; ++i) {
        const uint8_t* p = text_bytes + offsets[i];
        const uint8_t* end = text_bytes + offsets[i + 1];
        if ((size_t)(end - p) > kHashEmbedMaxTextBytes) return i;
        bool ascii = true;
        for (const uint8_t* q = p; q < end; ++q)
            if (*q >= 0x80) {
                ascii = false;
                break;
            }
        if (ascii) continue;
        if (!has_bitmap || !well_formed_utf8(p, end)) return i;
    }
    return HashEmbedder::kNoBadText;
}

HashEmbedder::~HashEmbedder() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    for (hipEvent_t ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (stream_) (void)hipStreamDestroy(stream_);
    for (DeviceBuffer* b : {&bitmap_, &text_, &offsets_, &counts_, &out_}) b->release();
}

SearchError HashEmbedder::init(int device, uint32_t dimension, int32_t algorithm, uint64_t seed, const uint8_t* alnum_bitmap_or_null) {
    if (dimension == 0) return make_error(FSGPU_ERR_INVALID_CONFIG, "dimension must be > 0");
    if (dimension > kHashEmbedMaxDim)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "dimension must be at most " + std::to_string(kHashEmbedMaxDim));
    if (algorithm != FSGPU_HASH_FNV_MODULAR && algorithm != FSGPU_HASH_JL_PROJECTION)
        return make_error(FSGPU_ERR_INVALID_CONFIG, "algorithm must be FSGPU_HASH_FNV_MODULAR or FSGPU_HASH_JL_PROJECTION");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return make_error(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (device < 0 || device >= count) return make_error(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
    FSGPU_HIP(hipSetDevice(device));
    device_ = device;
    dim_ = dimension;
    jl_ = algorithm == FSGPU_HASH_JL_PROJECTION;
    seed_ = seed;
    {
        // a short kernel next to the scans' chip-filling launches on other streams: highest priority (as Model2VecEmbedder)
        int least = 0, greatest = 0;
        FSGPU_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        FSGPU_HIP(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest));
    }
    if (alnum_bitmap_or_null) {
        FSGPU_TRY(bitmap_.reserve(kHashEmbedBitmapBytes));
        FSGPU_HIP(hipMemcpy(bitmap_.ptr, alnum_bitmap_or_null, kHashEmbedBitmapBytes, hipMemcpyHostToDevice));
        has_bitmap_ = true;
    }
    return ok();
}

SearchError HashEmbedder::embed_batch(const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out, float* out_dev,
                                      uint32_t* out_token_counts, uint32_t* out_bad_text, float* stage_ms) {
    if (out_bad_text) *out_bad_text = kNoBadText;
    if (n == 0) return ok();
    if (!offsets || (!out && !out_dev)) return make_error(FSGPU_ERR_NULL_ARGUMENT, "offsets/out is null");
    for (uint32_t i = 0; i < n; ++i)
        if (offsets[i + 1] < offsets[i]) return make_error(FSGPU_ERR_INVALID_CONFIG, "offsets must be non-decreasing");
    const uint32_t total = offsets[n];   // the byte buffer's length: every offset is within it
    if (total && !text_bytes) return make_error(FSGPU_ERR_NULL_ARGUMENT, "text_bytes is null");
    const uint32_t bad = hash_embed_first_bad_text(text_bytes, offsets, n, has_bitmap_);
    if (bad != kNoBadText) {
        if (out_bad_text) *out_bad_text = bad;
        if (offsets[bad + 1] - offsets[bad] > kHashEmbedMaxTextBytes)
            return make_error(FSGPU_ERR_INVALID_CONFIG, "text " + std::to_string(bad) + " is longer than 32 MiB");
        return make_error(FSGPU_ERR_INVALID_CONFIG,
                          "text " + std::to_string(bad) +
                              (has_bitmap_ ? " is not well-formed UTF-8" : " holds a byte >= 0x80 and the embedder has no alphanumeric table"));
    }
    // staging buffers and the stream are per handle: concurrent callers take turns (fsgpu.h: calls on one handle serialise)
    std::lock_guard<std::mutex> lock(mu_);
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(text_.reserve(total ? total : 1));
    FSGPU_TRY(offsets_.reserve((size_t)(n + 1) * 4));
    FSGPU_TRY(counts_.reserve((size_t)n * 4));
    if (!out_dev) FSGPU_TRY(out_.reserve((size_t)n * dim_ * 4));
    if (stage_ms) {
        for (hipEvent_t& ev : ev_)
            if (!ev) FSGPU_HIP(hipEventCreate(&ev));
        FSGPU_HIP(hipEventRecord(ev_[0], stream_));
    }
    if (total) FSGPU_HIP(hipMemcpyAsync(text_.ptr, text_bytes, total, hipMemcpyHostToDevice, stream_));
    FSGPU_HIP(hipMemcpyAsync(offsets_.ptr, offsets, (size_t)(n + 1) * 4, hipMemcpyHostToDevice, stream_));
    HashEmbedArgs a;
    a.text = static_cast<const uint8_t*>(text_.ptr);
    a.offsets = static_cast<const uint32_t*>(offsets_.ptr);
    a.bitmap = has_bitmap_ ? static_cast<const uint8_t*>(bitmap_.ptr) : nullptr;
    a.out = out_dev ? out_dev : static_cast<float*>(out_.ptr);   // (device output: the vectors stay in HBM)
    a.token_counts = static_cast<uint32_t*>(counts_.ptr);
    a.seed = seed_;
    a.dim = dim_;
    if (stage_ms) FSGPU_HIP(hipEventRecord(ev_[1], stream_));
    FSGPU_HIP(launch_hash_embed(a, n, jl_, stream_));
    if (stage_ms) FSGPU_HIP(hipEventRecord(ev_[2], stream_));
    if (out) FSGPU_HIP(hipMemcpyAsync(out, a.out, (size_t)n * dim_ * 4, hipMemcpyDeviceToHost, stream_));
    if (out_token_counts) FSGPU_HIP(hipMemcpyAsync(out_token_counts, counts_.ptr, (size_t)n * 4, hipMemcpyDeviceToHost, stream_));
    if (stage_ms) FSGPU_HIP(hipEventRecord(ev_[3], stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    if (stage_ms)
        for (int i = 0; i < 3; ++i) FSGPU_HIP(hipEventElapsedTime(&stage_ms[i], ev_[i], ev_[i + 1]));
    return ok();
}

}  // namespace fsgpu

// hash_embedder.hpp — HashEmbedder (crates/frankensearch-embed/src/hash_embedder.rs:201-328) on the device: raw text bytes in,
// L2-normalised vectors out (hash_embed_kernels.hip).  No weights: the only data is the caller's table of
// alphanumeric code points (char::is_alphanumeric of the host's toolchain), one bit per code point.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>

#include "vector_index.hpp"

namespace fsgpu {

constexpr uint32_t kHashEmbedMaxDim = 1024;              // 16 integer accumulators per lane of the JL kernel
constexpr uint32_t kHashEmbedChunkStates = 1024;         // token states the JL kernel's LDS list holds between flushes
constexpr uint32_t kHashEmbedCodePoints = 0x110000;      // bits of the alphanumeric table
constexpr uint32_t kHashEmbedBitmapBytes = kHashEmbedCodePoints / 8;
constexpr uint32_t kHashEmbedMaxTextBytes = 32u << 20;   // < 2^24 tokens: where the integer-exactness argument ends (:294-298)

struct HashEmbedArgs {
    const uint8_t* text;        // the texts' bytes back to back (device)
    const uint32_t* offsets;    // [n + 1] (device): text i owns text[offsets[i], offsets[i + 1])
    const uint8_t* bitmap;      // kHashEmbedBitmapBytes (device) or null: bit c = code point c is alphanumeric
    float* out;                 // [n, dim]
    uint32_t* token_counts;     // [n] tokens hashed per text, may be null
    u64 seed;                   // JLProjection { seed }
    uint32_t dim;
};
hipError_t launch_hash_embed(const HashEmbedArgs& args, uint32_t n, bool jl, hipStream_t stream);

class HashEmbedder {
  public:
    static constexpr uint32_t kNoBadText = 0xffffffffu;
    ~HashEmbedder();
    // dimension and algorithm are judged before a device is looked for
    SearchError init(int device, uint32_t dimension, int32_t algorithm, uint64_t seed, const uint8_t* alnum_bitmap_or_null);
    // out_dev (on this embedder's device, may be null): the vectors are left in device memory; out (may then be null): host copy.
    // A refused text (a byte >= 0x80 without a table, ill-formed UTF-8 with one, longer than 32 MiB) is named in *out_bad_text
    // and nothing is written.  stage_ms (lab timing, may be null): the device's own time between events on the stream for
    // {the copies in, the kernel, the copies out}.
    SearchError embed_batch(const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out, float* out_dev,
                            uint32_t* out_token_counts, uint32_t* out_bad_text, float* stage_ms = nullptr);
    uint32_t dimension() const { return dim_; }
    int device() const { return device_; }

  private:
    std::mutex mu_;
    int device_ = -1;
    uint32_t dim_ = 0;
    bool jl_ = false, has_bitmap_ = false;
    uint64_t seed_ = 0;
    DeviceBuffer bitmap_, text_, offsets_, counts_, out_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};   // lab timing only, created on first use
};

// The first text that HashEmbedder refuses, or HashEmbedder::kNoBadText: strict UTF-8 (what &str guarantees the reference: no
// overlong forms, no surrogates, nothing past U+10FFFF, no truncated sequence) when a table is present, ASCII only without one.
// offsets must already be non-decreasing.
uint32_t hash_embed_first_bad_text(const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, bool has_bitmap);

}  // namespace fsgpu

// lab_guard.hpp — the host half of the lab stage harness (LabStage, fsgpu_lab_api.cpp): what a guarded output looks like and how it
// is checked once it is back on the host, the guard rows behind an uploaded slab, the padded bitmap.  No HIP header, no device call:
// tests/host/lab_guard_check.cpp compiles this file alone and checks it under the host sanitizers.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>

namespace fsgpu {
namespace lab {

constexpr int kGuardByte = 0xA5;
constexpr size_t kBand = 4096;   // the band of a byte-sized output; a row-shaped one has 64 rows of its own width

// One output of a stage on the device: [band | bytes | band], both bands of kGuardByte.
struct Out {
    unsigned char* base = nullptr;
    size_t band = 0, bytes = 0;
    void* host = nullptr;   // receives the body (slab_rows: [slabs][slab_rows][row]); null: nothing is copied
    size_t row = 0;         // bytes of one row (slab_rows only)
    size_t slab_rows = 0;   // non-zero: the body is slabs x 32 workspace rows, all guard bytes beforehand; rows slab_rows..31 of each must keep them
    bool untouched = false; // the launch must leave the whole body as it was filled (guard bytes; nothing goes to the host)
    bool widen = false;     // the body is f16 and the host wants f32: the caller widens, nothing is copied here
    void* ptr() const { return base + band; }
    size_t total() const { return bytes + 2 * band; }
};

// h: the o.total() bytes read back from o.base.  Copies the body to o.host as o says; true when a byte that had to keep kGuardByte did not.
inline bool collect_out(const Out& o, const unsigned char* h) {
    bool hit = false;
    const unsigned char* body = h + o.band;
    for (size_t i = 0; i < o.band; ++i)
        if (h[i] != kGuardByte || body[o.bytes + i] != kGuardByte) hit = true;
    if (o.untouched) {
        for (size_t i = 0; i < o.bytes; ++i)
            if (body[i] != kGuardByte) hit = true;
    } else if (o.slab_rows) {
        for (size_t sl = 0; sl < o.bytes / (32 * o.row); ++sl) {
            const unsigned char* slab = body + sl * 32 * o.row;
            std::memcpy(static_cast<unsigned char*>(o.host) + sl * o.slab_rows * o.row, slab, o.slab_rows * o.row);
            for (size_t i = o.slab_rows * o.row; i < 32 * o.row; ++i)
                if (slab[i] != kGuardByte) hit = true;
        }
    } else if (!o.widen && o.host) {
        std::memcpy(o.host, body, o.bytes);
    }
    return hit;
}

// What lies behind the last row of an uploaded slab (or behind the last valid query), so that a read past the end shows in the answers.
enum class Tail { kF16NaN, kF32NaN, kByte7f };   // 0x7e00 halves, 0x7fc00000 words, 0x7f bytes (int8, 4-bit)

// `body` bytes of src followed by `tail` bytes of the pattern.
inline std::vector<unsigned char> with_guard_tail(const void* src, size_t body, size_t tail, Tail t) {
    std::vector<unsigned char> h(body + tail, 0x7f);
    std::memcpy(h.data(), src, body);
    unsigned char* g = h.data() + body;
    if (t == Tail::kF16NaN)
        for (size_t i = 0; i + 1 < tail; i += 2) g[i] = 0x00, g[i + 1] = 0x7e;
    else if (t == Tail::kF32NaN)
        for (size_t i = 0; i + 3 < tail; i += 4) g[i] = 0, g[i + 1] = 0, g[i + 2] = 0xc0, g[i + 3] = 0x7f;
    return h;
}

inline size_t bitmap_words(size_t nrows) { return (nrows + 63) / 64; }

// The host copy of a live / allow bitmap with two zero words behind the last.
inline std::vector<uint64_t> padded_bitmap(const uint64_t* src, size_t words) {
    std::vector<uint64_t> w(words + 2, 0);
    std::memcpy(w.data(), src, words * 8);
    return w;
}

}  // namespace lab
}  // namespace fsgpu

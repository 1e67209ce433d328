// wordpiece.hpp — the BERT WordPiece tokenizer on the device: raw text bytes in, token ids out as a dense CSR
// (wordpiece_kernels.hip).  BertNormalizer and BertPreTokenizer live in the caller's per-code-point table
// (include/fsgpu.h), the vocabulary in an open-addressing hash table built here on the host.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <mutex>
#include <vector>

#include "../../include/fsgpu.h"
#include "vector_index.hpp"

namespace fsgpu {

constexpr uint32_t kWpMaxWordChars = 1024;     // upper end of max_input_chars_per_word
constexpr uint32_t kWpMaxPrefixBytes = 16;
constexpr uint32_t kWpMaxAdded = 32;           // added tokens, each of 1..32 bytes
constexpr uint32_t kWpMaxAddedBytes = 32;
constexpr uint32_t kWpHashMul = 0x01000193u;   // the polynomial hash's base (odd: arithmetic modulo 2^32)
constexpr uint32_t kWpPowCount = 4 * kWpMaxWordChars + kWpMaxPrefixBytes + 1;   // powers a piece's byte length can ask for
constexpr uint32_t kWpEmptySlot = 0xffffffffu;

// What the kernels read; every pointer is device memory.
struct WordPieceTables {
    const uint32_t* cp_info;      // [0x110000]
    const uint32_t* expansions;   // [expansions_len]
    const uint8_t* vocab_bytes;
    const uint32_t* vocab_offsets;   // [vocab_size + 1]
    const uint2* slots;           // [slot_mask + 1] {hash, id}; id == kWpEmptySlot: empty
    const uint32_t* pow;          // [kWpPowCount] kWpHashMul^k
    const uint8_t* added_bytes;
    const uint32_t* added_offsets;   // [added_count + 1]
    uint32_t expansions_len, vocab_size, slot_mask, probe_bound;
    uint32_t added_count, unk_id, cls_id, sep_id, max_chars;
    uint32_t prefix_hash, prefix_len;
    uint8_t prefix[kWpMaxPrefixBytes];
};

struct WordPieceTokenizeArgs {
    const WordPieceTables* t;     // (device memory: read where needed, not held in registers from the kernel's start)
    uint32_t max_chars;           // t->max_chars, for the launch's LDS size
    const uint8_t* text;          // the texts' bytes back to back
    const uint32_t* offsets;      // [n + 1]
    const uint32_t* piece_base;   // [n + 1]: text i may keep piece_base[i + 1] - piece_base[i] pieces, at pieces[piece_base[i]..]
    uint32_t* pieces;
    uint32_t* counts;             // [n] pieces the text has (before truncation)
    uint8_t* flagged;             // [n] 1: added-token content or a HOST code point
};

struct WordPieceAssembleArgs {
    const uint32_t* piece_base;   // [texts + 1]
    const uint32_t* pieces;
    const uint32_t* counts;       // [texts]
    const uint8_t* flagged;       // [texts]
    uint32_t* keep;               // [texts] pieces of each text that go out (written by the offsets kernel)
    uint32_t* out_offsets;        // [n + 1]
    uint8_t* out_status;          // [n]
    unsigned long long* out_total;
    uint32_t* out_ids;
    uint32_t* out_type_ids;       // pairs only
    uint32_t n;                   // sequences: texts (single) or pairs (texts = 2 n: the a texts, then the b texts)
    uint32_t max_length, add_special, cls_id, sep_id;
    bool pairs;
};

hipError_t launch_wordpiece_tokenize(const WordPieceTokenizeArgs& args, uint32_t texts, hipStream_t stream);
hipError_t launch_wordpiece_offsets(const WordPieceAssembleArgs& args, hipStream_t stream);
hipError_t launch_wordpiece_assemble(const WordPieceAssembleArgs& args, hipStream_t stream);
// the hand-off to the MiniLM short-text forward: row_id_dev [nblocks * 32] from the device ids and the blocks' first tokens
hipError_t launch_wordpiece_block_rows(const int32_t* ids_dev, const uint32_t* blk_tok_dev, int32_t* row_id_dev, uint32_t nblocks,
                                       hipStream_t stream);

// The same polynomial hash the kernels build from prefix hashes: h = h * kWpHashMul + byte, modulo 2^32.
inline uint32_t wordpiece_hash(const uint8_t* p, size_t len, uint32_t h = 0) {
    for (size_t i = 0; i < len; ++i) h = h * kWpHashMul + p[i];
    return h;
}
__host__ __device__ inline uint32_t wordpiece_slot(uint32_t h) { return (h ^ (h >> 15)) * 0x9e3779b1u; }   // (masked by the caller)

class WordPieceTokenizer {
  public:
    static constexpr uint32_t kNoBadText = 0xffffffffu;
    ~WordPieceTokenizer();
    // The config is judged completely before a device is looked for.
    static SearchError validate(const fsgpu_wordpiece_config& c);
    SearchError init(int device, const fsgpu_wordpiece_config& c);

    struct Request {
        const uint8_t* a_bytes = nullptr;
        const uint32_t* a_offsets = nullptr;
        const uint8_t* b_bytes = nullptr;    // pairs only
        const uint32_t* b_offsets = nullptr;
        uint32_t n = 0;
        bool pairs = false;
        bool add_special = false;
        uint32_t max_length = 0;
        uint64_t ids_capacity = 0;
        bool device_out = false;             // out_ids / out_type_ids / out_offsets are device memory
        uint32_t* out_ids = nullptr;
        uint32_t* out_type_ids = nullptr;
        uint32_t* out_offsets = nullptr;
        uint32_t* host_offsets = nullptr;    // device_out: a host copy of the offsets [n + 1] as well, nullable
        uint8_t* out_status = nullptr;       // host, nullable
        uint64_t* out_total = nullptr;       // host, nullable
        uint32_t* out_bad_text = nullptr;    // host, nullable
        float* stage_ms = nullptr;           // lab timing, nullable: {copies in, kernels, copies out} between events on the stream
        bool refuse_flagged = false;         // a flagged text fails the call and names itself in *out_bad_text
    };
    SearchError encode(const Request& r);

    // What a fused call hands to its encoder: the CSR in this tokenizer's own device buffers, and the offsets on the host as well
    // (an encoder plans its launches from the lengths; the ids stay where they are).
    struct OwnCsr {
        const uint32_t* ids_dev;
        const uint32_t* type_ids_dev;    // pairs only
        const uint32_t* offsets_dev;     // [n + 1]
        const uint32_t* offsets_host;    // [n + 1]
        uint64_t total;
    };
    // The fused calls: `r` names the texts (or pairs), add_special, max_length and out_bad_text; they are tokenised into the
    // tokenizer's own buffers and the CSR goes to `consume` while the tokenizer is still locked.  A flagged text is refused before
    // `consume` runs.  r.n must not be 0.
    template <typename F>
    SearchError encode_then(Request r, F consume) {
        std::lock_guard<std::mutex> lock(mu_);
        uint64_t total = 0;
        SearchError e = encode_own(r, &total);
        if (!e.ok()) return e;
        return consume(OwnCsr{static_cast<const uint32_t*>(own_ids_.ptr), static_cast<const uint32_t*>(own_types_.ptr),
                              static_cast<const uint32_t*>(own_offsets_.ptr), h_out_offsets_.data(), total});
    }

    int device() const { return device_; }
    uint32_t vocab_size() const { return tables_.vocab_size; }

  private:
    SearchError encode_locked(const Request& r);
    SearchError encode_own(Request& r, uint64_t* total);

    std::mutex mu_;
    int device_ = -1;
    WordPieceTables tables_{};
    DeviceBuffer tables_dev_, cp_info_, expansions_, vocab_bytes_, vocab_offsets_, slots_, pow_, added_bytes_, added_offsets_;
    DeviceBuffer text_, offsets_, piece_base_, pieces_, counts_, flagged_, keep_, out_offsets_, out_status_, out_total_, out_ids_,
        out_types_, own_ids_, own_types_, own_offsets_;
    std::vector<uint32_t> h_offsets_, h_piece_base_, h_out_offsets_;
    std::vector<uint8_t> h_status_;
    hipStream_t stream_ = nullptr;
    hipEvent_t ev_[4] = {nullptr, nullptr, nullptr, nullptr};   // lab timing only, created on first use
};

}  // namespace fsgpu

// wordpiece.cpp — host side of the device WordPiece tokenizer (wordpiece.hpp).
//
// The whole config is judged here before a device is looked for; the vocabulary's open-addressing table is built here and
// uploaded once with the caller's tables.  Everything a text can be refused for (offsets, strict UTF-8, the 32 MiB bound) is
// decided before a kernel is launched, by the hash embedder's validation.
#include "wordpiece.hpp"

#include <cstring>
#include <string>
#include <string_view>
#include <unordered_set>

#include "hash_embedder.hpp"
#include "vector_index_internal.hpp"

namespace fsgpu {

using namespace detail;

namespace {

SearchError bad(const std::string& what) { return make_error(FSGPU_ERR_INVALID_CONFIG, what); }

uint32_t utf8_len(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }

}  // namespace

SearchError WordPieceTokenizer::validate(const fsgpu_wordpiece_config& c) {
    for (uint32_t r : c.reserved)
        if (r != 0) return bad("reserved words must be 0");
    if (c.vocab_size == 0) return bad("the vocabulary is empty");
    if (!c.vocab_offsets || !c.cp_info) return make_error(FSGPU_ERR_NULL_ARGUMENT, "vocab_offsets / cp_info is null");
    if (c.max_input_chars_per_word == 0 || c.max_input_chars_per_word > kWpMaxWordChars)
        return bad("max_input_chars_per_word must be 1..1024");
    if (c.prefix_len > kWpMaxPrefixBytes) return bad("the continuing-subword prefix is longer than 16 bytes");
    if (c.prefix_len && !c.prefix_bytes) return make_error(FSGPU_ERR_NULL_ARGUMENT, "prefix_bytes is null");
    if (c.unk_id >= c.vocab_size || c.cls_id >= c.vocab_size || c.sep_id >= c.vocab_size)
        return bad("unk_id, cls_id and sep_id must be below vocab_size");
    if (c.vocab_offsets[0] != 0) return bad("vocab_offsets must start at 0");
    for (uint32_t i = 0; i < c.vocab_size; ++i)
        if (c.vocab_offsets[i + 1] < c.vocab_offsets[i]) return bad("vocab_offsets must be non-decreasing");
    if (c.vocab_offsets[c.vocab_size] && !c.vocab_bytes) return make_error(FSGPU_ERR_NULL_ARGUMENT, "vocab_bytes is null");
    if (c.added_count > kWpMaxAdded) return bad("more than 32 added tokens");
    if (c.added_count) {
        if (!c.added_offsets || !c.added_bytes) return make_error(FSGPU_ERR_NULL_ARGUMENT, "added_offsets / added_bytes is null");
        if (c.added_offsets[0] != 0) return bad("added_offsets must start at 0");
        for (uint32_t i = 0; i < c.added_count; ++i) {
            if (c.added_offsets[i + 1] < c.added_offsets[i]) return bad("added_offsets must be non-decreasing");
            const uint32_t len = c.added_offsets[i + 1] - c.added_offsets[i];
            if (len == 0 || len > kWpMaxAddedBytes) return bad("an added token must hold 1..32 bytes");
        }
    }
    if (c.expansions_len > FSGPU_WP_VALUE_MASK) return bad("expansions_len does not fit an index");
    if (c.expansions_len && !c.expansions) return make_error(FSGPU_ERR_NULL_ARGUMENT, "expansions is null");
    for (uint32_t i = 0; i < c.expansions_len; ++i)
        if (c.expansions[i] >= FSGPU_WP_CODE_POINTS) return bad("an expansion is not a code point");
    for (uint32_t cp = 0; cp < FSGPU_WP_CODE_POINTS; ++cp) {
        const uint32_t info = c.cp_info[cp];
        if (info >> 27) return bad("cp_info[" + std::to_string(cp) + "] has bits 27..31 set");
        const uint32_t len = (info >> FSGPU_WP_LEN_SHIFT) & FSGPU_WP_LEN_MASK, value = info & FSGPU_WP_VALUE_MASK;
        if (len > 3) return bad("cp_info[" + std::to_string(cp) + "] has an output length above 3");
        if (len == 1 && value >= FSGPU_WP_CODE_POINTS) return bad("cp_info[" + std::to_string(cp) + "] does not name a code point");
        if (len >= 2 && (uint64_t)value + len > c.expansions_len)
            return bad("cp_info[" + std::to_string(cp) + "] has an expansion index out of range");
    }
    std::unordered_set<std::string_view> seen;
    seen.reserve((size_t)c.vocab_size * 2);
    for (uint32_t i = 0; i < c.vocab_size; ++i) {
        const uint32_t len = c.vocab_offsets[i + 1] - c.vocab_offsets[i];
        const std::string_view s(len ? reinterpret_cast<const char*>(c.vocab_bytes) + c.vocab_offsets[i] : "", len);
        if (!seen.insert(s).second) return bad("vocabulary entries " + std::to_string(i) + " and an earlier one are equal");
    }
    return ok();
}

WordPieceTokenizer::~WordPieceTokenizer() {
    if (device_ >= 0) (void)hipSetDevice(device_);
    for (hipEvent_t ev : ev_)
        if (ev) (void)hipEventDestroy(ev);
    if (stream_) (void)hipStreamDestroy(stream_);
    for (DeviceBuffer* b : {&tables_dev_, &cp_info_, &expansions_, &vocab_bytes_, &vocab_offsets_, &slots_, &pow_, &added_bytes_, &added_offsets_, &text_,
                            &offsets_, &piece_base_, &pieces_, &counts_, &flagged_, &keep_, &out_offsets_, &out_status_, &out_total_,
                            &out_ids_, &out_types_, &own_ids_, &own_types_, &own_offsets_})
        b->release();
}

SearchError WordPieceTokenizer::init(int device, const fsgpu_wordpiece_config& c) {
    FSGPU_TRY(validate(c));
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0)
        return make_error(FSGPU_ERR_NO_DEVICE, "no HIP device visible (libfsgpu has no CPU fallback)");
    if (device < 0 || device >= count) return bad("device ordinal out of range");
    FSGPU_HIP(hipSetDevice(device));
    device_ = device;
    {
        int least = 0, greatest = 0;   // short kernels next to the scans' chip-filling launches: highest priority (as the embedders)
        FSGPU_HIP(hipDeviceGetStreamPriorityRange(&least, &greatest));
        FSGPU_HIP(hipStreamCreateWithPriority(&stream_, hipStreamNonBlocking, greatest));
    }
    // ---- the vocabulary's hash table: open addressing, linear probing, at most half full; the longest probe run is recorded ----
    uint32_t slots = 16;
    while (slots < 2u * c.vocab_size) slots <<= 1;
    std::vector<uint2> table(slots, uint2{0u, kWpEmptySlot});
    uint32_t probe_bound = 0;
    const uint32_t longest = 4 * kWpMaxWordChars + kWpMaxPrefixBytes;   // no piece of a word has more bytes
    for (uint32_t id = 0; id < c.vocab_size; ++id) {
        const uint32_t len = c.vocab_offsets[id + 1] - c.vocab_offsets[id];
        if (len == 0 || len > longest) continue;   // (never a piece)
        const uint32_t h = wordpiece_hash(c.vocab_bytes + c.vocab_offsets[id], len);
        uint32_t at = wordpiece_slot(h) & (slots - 1), probe = 0;
        while (table[at].y != kWpEmptySlot) {
            at = (at + 1) & (slots - 1);
            ++probe;
        }
        table[at] = uint2{h, id};
        if (probe > probe_bound) probe_bound = probe;
    }
    std::vector<uint32_t> pow(kWpPowCount);
    pow[0] = 1;
    for (uint32_t i = 1; i < kWpPowCount; ++i) pow[i] = pow[i - 1] * kWpHashMul;
    // the table as the kernels read it: an entry longer than its code point's UTF-8 form is the host's (include/fsgpu.h)
    std::vector<uint32_t> info(c.cp_info, c.cp_info + FSGPU_WP_CODE_POINTS);
    for (uint32_t cp = 0; cp < FSGPU_WP_CODE_POINTS; ++cp) {
        const uint32_t len = (info[cp] >> FSGPU_WP_LEN_SHIFT) & FSGPU_WP_LEN_MASK;
        if (len > (utf8_len(cp) > 3u ? 3u : utf8_len(cp))) info[cp] |= FSGPU_WP_HOST;
    }
    auto upload = [&](DeviceBuffer& dst, const void* src, size_t bytes) -> SearchError {
        FSGPU_TRY(dst.reserve(bytes ? bytes : 4));
        if (bytes) FSGPU_HIP(hipMemcpy(dst.ptr, src, bytes, hipMemcpyHostToDevice));
        return ok();
    };
    const uint32_t added_bytes = c.added_count ? c.added_offsets[c.added_count] : 0;
    const uint32_t zero = 0;
    FSGPU_TRY(upload(cp_info_, info.data(), info.size() * 4));
    FSGPU_TRY(upload(expansions_, c.expansions, (size_t)c.expansions_len * 4));
    FSGPU_TRY(upload(vocab_bytes_, c.vocab_bytes, c.vocab_offsets[c.vocab_size]));
    FSGPU_TRY(upload(vocab_offsets_, c.vocab_offsets, (size_t)(c.vocab_size + 1) * 4));
    FSGPU_TRY(upload(slots_, table.data(), table.size() * sizeof(uint2)));
    FSGPU_TRY(upload(pow_, pow.data(), pow.size() * 4));
    FSGPU_TRY(upload(added_bytes_, c.added_bytes, added_bytes));
    FSGPU_TRY(upload(added_offsets_, c.added_count ? c.added_offsets : &zero, (size_t)(c.added_count + 1) * 4));
    WordPieceTables& t = tables_;
    t.cp_info = static_cast<const uint32_t*>(cp_info_.ptr);
    t.expansions = static_cast<const uint32_t*>(expansions_.ptr);
    t.vocab_bytes = static_cast<const uint8_t*>(vocab_bytes_.ptr);
    t.vocab_offsets = static_cast<const uint32_t*>(vocab_offsets_.ptr);
    t.slots = static_cast<const uint2*>(slots_.ptr);
    t.pow = static_cast<const uint32_t*>(pow_.ptr);
    t.added_bytes = static_cast<const uint8_t*>(added_bytes_.ptr);
    t.added_offsets = static_cast<const uint32_t*>(added_offsets_.ptr);
    t.expansions_len = c.expansions_len;
    t.vocab_size = c.vocab_size;
    t.slot_mask = slots - 1;
    t.probe_bound = probe_bound;
    t.added_count = c.added_count;
    t.unk_id = c.unk_id;
    t.cls_id = c.cls_id;
    t.sep_id = c.sep_id;
    t.max_chars = c.max_input_chars_per_word;
    t.prefix_len = c.prefix_len;
    t.prefix_hash = wordpiece_hash(c.prefix_bytes, c.prefix_len);
    std::memset(t.prefix, 0, sizeof(t.prefix));
    if (c.prefix_len) std::memcpy(t.prefix, c.prefix_bytes, c.prefix_len);
    FSGPU_TRY(upload(tables_dev_, &tables_, sizeof(tables_)));
    return ok();
}

SearchError WordPieceTokenizer::encode(const Request& r) {
    std::lock_guard<std::mutex> lock(mu_);
    return encode_locked(r);
}

SearchError WordPieceTokenizer::encode_own(Request& r, uint64_t* total) {
    if (r.out_bad_text) *r.out_bad_text = kNoBadText;
    *total = 0;
    const uint32_t n = r.n;
    if (n == 0 || !r.a_offsets || (r.pairs && !r.b_offsets)) return make_error(FSGPU_ERR_NULL_ARGUMENT, "offsets is null");
    // (pieces never outnumber bytes; up to three special tokens per sequence.  Decreasing offsets are refused by encode_locked.)
    uint64_t room = (uint64_t)(r.pairs ? 3 : 2) * n;
    if (r.a_offsets[n] >= r.a_offsets[0]) room += r.a_offsets[n] - r.a_offsets[0];
    if (r.pairs && r.b_offsets[n] >= r.b_offsets[0]) room += r.b_offsets[n] - r.b_offsets[0];
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(own_ids_.reserve(room * 4));
    if (r.pairs) FSGPU_TRY(own_types_.reserve(room * 4));
    FSGPU_TRY(own_offsets_.reserve((size_t)(n + 1) * 4));
    h_out_offsets_.resize((size_t)n + 1);
    r.ids_capacity = room;
    r.device_out = true;
    r.out_ids = static_cast<uint32_t*>(own_ids_.ptr);
    r.out_type_ids = static_cast<uint32_t*>(own_types_.ptr);
    r.out_offsets = static_cast<uint32_t*>(own_offsets_.ptr);
    r.host_offsets = h_out_offsets_.data();
    r.out_status = nullptr;
    r.out_total = total;
    r.refuse_flagged = true;
    return encode_locked(r);
}

SearchError WordPieceTokenizer::encode_locked(const Request& r) {
    if (r.out_bad_text) *r.out_bad_text = kNoBadText;
    const uint32_t n = r.n;
    if (n && (!r.a_offsets || (r.pairs && !r.b_offsets))) return make_error(FSGPU_ERR_NULL_ARGUMENT, "offsets is null");
    if (!r.out_offsets || (n && (!r.out_ids || (r.pairs && !r.out_type_ids))))
        return make_error(FSGPU_ERR_NULL_ARGUMENT, "out_ids / out_type_ids / out_offsets is null");
    if (n > 0x3fffffffu) return bad("too many texts in one call");
    const uint32_t special = r.pairs ? 3u : (r.add_special ? 2u : 0u);
    if (r.max_length != 0 && r.max_length < special) return bad("max_length is below the special tokens' count");
    if (n == 0) {
        if (r.out_total) *r.out_total = 0;
        if (r.device_out) {
            FSGPU_HIP(hipSetDevice(device_));
            FSGPU_HIP(hipMemsetAsync(r.out_offsets, 0, 4, stream_));
            FSGPU_HIP(hipStreamSynchronize(stream_));
        } else {
            r.out_offsets[0] = 0;
        }
        return ok();
    }
    // ---- what a text can be refused for, before anything is launched ----
    const int sides = r.pairs ? 2 : 1;
    const uint8_t* side_bytes[2] = {r.a_bytes, r.b_bytes};
    const uint32_t* side_offsets[2] = {r.a_offsets, r.b_offsets};
    uint32_t first_bad = kNoBadText;
    uint64_t total_bytes = 0;
    for (int s = 0; s < sides; ++s) {
        const uint32_t* off = side_offsets[s];
        for (uint32_t i = 0; i < n; ++i)
            if (off[i + 1] < off[i]) return bad("offsets must be non-decreasing");
        if (off[n] && !side_bytes[s]) return make_error(FSGPU_ERR_NULL_ARGUMENT, "text_bytes is null");
        total_bytes += off[n] - off[0];
        const uint32_t b = hash_embed_first_bad_text(side_bytes[s], off, n, true);
        if (b < first_bad) first_bad = b;
    }
    if (first_bad != kNoBadText) {
        if (r.out_bad_text) *r.out_bad_text = first_bad;
        return bad("text " + std::to_string(first_bad) + " is not well-formed UTF-8 or is longer than 32 MiB");
    }
    if (total_bytes > 0xffffffffull) return bad("a call's texts must stay below 4 GiB");
    // ---- texts (the a texts, then the b texts) rebased to one buffer; the room each may fill in the piece buffer ----
    const uint32_t texts = n * (uint32_t)sides;
    const uint32_t keep_max = r.max_length ? r.max_length - special : 0xffffffffu;
    h_offsets_.resize((size_t)texts + 1);
    h_piece_base_.resize((size_t)texts + 1);
    h_offsets_[0] = 0;
    h_piece_base_[0] = 0;
    for (int s = 0; s < sides; ++s)
        for (uint32_t i = 0; i < n; ++i) {
            const uint32_t len = side_offsets[s][i + 1] - side_offsets[s][i];
            const size_t k = (size_t)s * n + i;
            h_offsets_[k + 1] = h_offsets_[k] + len;
            h_piece_base_[k + 1] = h_piece_base_[k] + (len < keep_max ? len : keep_max);   // (pieces never outnumber bytes)
        }
    const uint32_t piece_room = h_piece_base_[texts];
    FSGPU_HIP(hipSetDevice(device_));
    FSGPU_TRY(text_.reserve(total_bytes ? total_bytes : 1));
    FSGPU_TRY(offsets_.reserve((size_t)(texts + 1) * 4));
    FSGPU_TRY(piece_base_.reserve((size_t)(texts + 1) * 4));
    FSGPU_TRY(pieces_.reserve((size_t)(piece_room ? piece_room : 1) * 4));
    FSGPU_TRY(counts_.reserve((size_t)texts * 4));
    FSGPU_TRY(flagged_.reserve(texts));
    FSGPU_TRY(keep_.reserve((size_t)texts * 4));
    FSGPU_TRY(out_offsets_.reserve((size_t)(n + 1) * 4));
    FSGPU_TRY(out_status_.reserve(n));
    FSGPU_TRY(out_total_.reserve(8));
    if (r.stage_ms) {
        for (hipEvent_t& ev : ev_)
            if (!ev) FSGPU_HIP(hipEventCreate(&ev));
        FSGPU_HIP(hipEventRecord(ev_[0], stream_));
    }
    {
        size_t at = 0;
        for (int s = 0; s < sides; ++s) {
            const uint32_t len = side_offsets[s][n] - side_offsets[s][0];
            if (len)
                FSGPU_HIP(hipMemcpyAsync(static_cast<uint8_t*>(text_.ptr) + at, side_bytes[s] + side_offsets[s][0], len, hipMemcpyHostToDevice,
                                         stream_));
            at += len;
        }
    }
    FSGPU_HIP(hipMemcpyAsync(offsets_.ptr, h_offsets_.data(), (size_t)(texts + 1) * 4, hipMemcpyHostToDevice, stream_));
    FSGPU_HIP(hipMemcpyAsync(piece_base_.ptr, h_piece_base_.data(), (size_t)(texts + 1) * 4, hipMemcpyHostToDevice, stream_));
    if (r.stage_ms) FSGPU_HIP(hipEventRecord(ev_[1], stream_));
    WordPieceTokenizeArgs ta;
    ta.t = static_cast<const WordPieceTables*>(tables_dev_.ptr);
    ta.max_chars = tables_.max_chars;
    ta.text = static_cast<const uint8_t*>(text_.ptr);
    ta.offsets = static_cast<const uint32_t*>(offsets_.ptr);
    ta.piece_base = static_cast<const uint32_t*>(piece_base_.ptr);
    ta.pieces = static_cast<uint32_t*>(pieces_.ptr);
    ta.counts = static_cast<uint32_t*>(counts_.ptr);
    ta.flagged = static_cast<uint8_t*>(flagged_.ptr);
    FSGPU_HIP(launch_wordpiece_tokenize(ta, texts, stream_));
    WordPieceAssembleArgs aa{};
    aa.piece_base = ta.piece_base;
    aa.pieces = ta.pieces;
    aa.counts = ta.counts;
    aa.flagged = ta.flagged;
    aa.keep = static_cast<uint32_t*>(keep_.ptr);
    aa.out_offsets = static_cast<uint32_t*>(out_offsets_.ptr);
    aa.out_status = static_cast<uint8_t*>(out_status_.ptr);
    aa.out_total = static_cast<unsigned long long*>(out_total_.ptr);
    aa.n = n;
    aa.max_length = r.max_length;
    aa.add_special = r.pairs || r.add_special ? 1u : 0u;
    aa.cls_id = tables_.cls_id;
    aa.sep_id = tables_.sep_id;
    aa.pairs = r.pairs;
    FSGPU_HIP(launch_wordpiece_offsets(aa, stream_));
    unsigned long long total = 0;
    h_status_.resize(n);
    FSGPU_HIP(hipMemcpyAsync(&total, out_total_.ptr, 8, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipMemcpyAsync(h_status_.data(), out_status_.ptr, n, hipMemcpyDeviceToHost, stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    if (r.refuse_flagged)
        for (uint32_t i = 0; i < n; ++i)
            if (h_status_[i]) {
                if (r.out_bad_text) *r.out_bad_text = i;
                return bad("text " + std::to_string(i) + " holds an added token's content or a code point the device table leaves to the host");
            }
    if (total > 0xffffffffull) return bad("a call's ids must stay below 2^32");
    if (r.out_total) *r.out_total = total;
    if (total > r.ids_capacity)
        return bad("ids_capacity " + std::to_string(r.ids_capacity) + " is too small: the call needs " + std::to_string(total));
    // ---- the ids, dense ----
    if (r.device_out) {
        aa.out_ids = r.out_ids;
        aa.out_type_ids = r.out_type_ids;
    } else {
        FSGPU_TRY(out_ids_.reserve((size_t)(total ? total : 1) * 4));
        aa.out_ids = static_cast<uint32_t*>(out_ids_.ptr);
        if (r.pairs) {
            FSGPU_TRY(out_types_.reserve((size_t)(total ? total : 1) * 4));
            aa.out_type_ids = static_cast<uint32_t*>(out_types_.ptr);
        }
    }
    FSGPU_HIP(launch_wordpiece_assemble(aa, stream_));
    if (r.stage_ms) FSGPU_HIP(hipEventRecord(ev_[2], stream_));
    if (r.device_out) {
        FSGPU_HIP(hipMemcpyAsync(r.out_offsets, out_offsets_.ptr, (size_t)(n + 1) * 4, hipMemcpyDeviceToDevice, stream_));
        if (r.host_offsets) FSGPU_HIP(hipMemcpyAsync(r.host_offsets, out_offsets_.ptr, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, stream_));
    } else {
        if (total) FSGPU_HIP(hipMemcpyAsync(r.out_ids, aa.out_ids, (size_t)total * 4, hipMemcpyDeviceToHost, stream_));
        if (total && r.pairs) FSGPU_HIP(hipMemcpyAsync(r.out_type_ids, aa.out_type_ids, (size_t)total * 4, hipMemcpyDeviceToHost, stream_));
        FSGPU_HIP(hipMemcpyAsync(r.out_offsets, out_offsets_.ptr, (size_t)(n + 1) * 4, hipMemcpyDeviceToHost, stream_));
    }
    if (r.stage_ms) FSGPU_HIP(hipEventRecord(ev_[3], stream_));
    FSGPU_HIP(hipStreamSynchronize(stream_));
    if (r.stage_ms)
        for (int i = 0; i < 3; ++i) FSGPU_HIP(hipEventElapsedTime(&r.stage_ms[i], ev_[i], ev_[i + 1]));
    if (r.out_status) std::memcpy(r.out_status, h_status_.data(), n);
    return ok();
}

}  // namespace fsgpu

// wordpiece_kernels.hip — BertNormalizer -> BertPreTokenizer -> WordPiece -> [CLS] ... [SEP] from raw text bytes (gfx950).
//
// Three launches per call:
//   wordpiece_tokenize_kernel  one workgroup of four waves per text.
//     A  lanes stride over the bytes; the lane on a character's first byte decodes it (every read clamped to the text), looks the
//        code point up in the caller's table and appends its 0..3 normalised code points, with their class (plain / separator /
//        word on its own), to an LDS window in text order (a workgroup prefix sum of the counts).  Every byte position is also
//        compared with the added tokens' contents; a match or a HOST code point flags the text.
//     B  word starts of the window are listed; one wave per word.  The word's UTF-8 prefix hashes come from a wave scan over
//        (multiplier, addend) pairs of a polynomial hash modulo 2^32, so the hash of any piece [start, end) follows from two
//        prefixes; the lanes are the candidate ends, longest first, each probes the open-addressing table (a hit is confirmed
//        byte by byte against the vocabulary blob), one __ballot picks the longest.  A piece lands in the LDS slot
//        word start + piece number (a word of L characters has at most L pieces), so word order is kept without a sort.
//     C  the slots are compacted in order (prefix sum again) into the text's region of the piece buffer, up to the pieces the
//        call can keep; the count runs on.
//     A text longer than the window is taken in windows: the words before the last word start are finished, the open word is
//     moved to the window's front.  An open word is cut at max_input_chars_per_word + 1 characters: it is [UNK] whatever follows.
//   wordpiece_offsets_kernel   one workgroup: pieces kept per text (truncation, the pair rule), exclusive sum -> CSR offsets.
//   wordpiece_assemble_kernel  one workgroup per sequence: [CLS] pieces [SEP] (and type ids for pairs) into the dense id array.
//   wordpiece_block_rows_kernel  the hand-off to the MiniLM short-text forward: its row blocks' ids from the device CSR.
// Every loop is bounded by the text's end, the window, the word cap or the table's recorded probe bound.
#include "wordpiece.hpp"

namespace fsgpu {

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr uint32_t kCap = 2048;                      // the LDS window, in normalised code points
// What one stride of bytes can append, as the kernel sees it: up to 3 per character.  The tables create() uploads never exceed
// one per byte (an entry longer than its code point's UTF-8 form is made HOST there), so 256 would do for them; the bound is kept
// at what the table's FORMAT allows, so that no table a host could hand over writes outside the window.
constexpr uint32_t kStrideOut = 3u * kThreads;
constexpr uint32_t kValue = FSGPU_WP_VALUE_MASK;
constexpr uint32_t kClsShift = 21;                   // window entries: code point | class << 21
constexpr uint32_t kPlain = 0, kSpace = 1, kIsolate = 2;
constexpr uint32_t kNone = 0xffffffffu;
constexpr int kOffsetThreads = 1024;

static_assert(kWpMaxWordChars + 1 + kStrideOut <= kCap, "a carried word and one more stride must fit the window");

// Exclusive prefix sum of v over the workgroup (waves of 64) in thread order, and the total.  Two barriers.
template <int WAVES>
__device__ __forceinline__ uint32_t block_exclusive(uint32_t v, uint32_t lane, uint32_t wave, uint32_t* wsum, uint32_t& total) {
    uint32_t inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t o = __shfl_up(inc, d);
        if (lane >= (uint32_t)d) inc += o;
    }
    if (lane == 63u) wsum[wave] = inc;
    __syncthreads();
    uint32_t base = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) {
        const uint32_t s = wsum[w];
        base += (uint32_t)w < wave ? s : 0u;
        tot += s;
    }
    __syncthreads();   // (wsum may be written again)
    total = tot;
    return base + inc - v;
}

// 32-bit words of a wave's share of the dynamic LDS
__host__ __device__ inline uint32_t wave_lds_words(uint32_t max_chars) { return (max_chars + 1u) + max_chars + (max_chars + 3u) / 2u; }

__device__ __forceinline__ uint32_t cls_of(uint32_t entry) { return entry >> kClsShift; }

__device__ __forceinline__ uint32_t utf8_len(uint32_t cp) { return cp < 0x80u ? 1u : cp < 0x800u ? 2u : cp < 0x10000u ? 3u : 4u; }

// byte k (k < utf8_len(cp)) of the code point's UTF-8 form
__device__ __forceinline__ uint32_t utf8_byte(uint32_t cp, uint32_t nb, uint32_t k) {
    if (nb == 1u) return cp;
    const uint32_t shift = 6u * (nb - 1u - k);
    if (k == 0u) return ((0xf00u >> nb) & 0xffu) | (cp >> shift);   // 110xxxxx / 1110xxxx / 11110xxx
    return 0x80u | ((cp >> shift) & 0x3fu);
}

// a word starts at window position j: not a separator, and at the front, on its own, or behind a separator / a word on its own
__device__ __forceinline__ bool word_starts(const uint32_t* norm, uint32_t j) {
    const uint32_t c = cls_of(norm[j]);
    if (c == kSpace) return false;
    return j == 0u || c == kIsolate || cls_of(norm[j - 1u]) != kPlain;
}

// the id of the piece [start, end) of the wave's word (with the continuing prefix when start > 0), or kNone
__device__ __forceinline__ uint32_t lookup_piece(const WordPieceTables& t, const uint32_t* ph, const uint16_t* bo, const uint8_t* wb,
                                                 uint32_t start, uint32_t end) {
    const uint32_t first = bo[start];
    const uint32_t nbytes = (uint32_t)bo[end] - first;
    const uint32_t pw = t.pow[nbytes];
    const uint32_t plen = start > 0u ? t.prefix_len : 0u;
    const uint32_t h = ph[end] - ph[start] * pw + (start > 0u ? t.prefix_hash * pw : 0u);
    const uint32_t want = nbytes + plen;
    const uint32_t slot = wordpiece_slot(h);
    uint32_t found = kNone;
    for (uint32_t probe = 0; probe <= t.probe_bound && found == kNone; ++probe) {
        const uint2 s = t.slots[(slot + probe) & t.slot_mask];
        if (s.y == kWpEmptySlot) break;
        if (s.x != h || s.y >= t.vocab_size) continue;
        const uint32_t vo = t.vocab_offsets[s.y];
        if (t.vocab_offsets[s.y + 1u] - vo != want) continue;
        const uint8_t* __restrict__ v = t.vocab_bytes + vo;
        uint32_t k = 0;   // a hit is confirmed byte by byte: a collision never gives an id
        while (k < want && (uint32_t)v[k] == (k < plen ? (uint32_t)t.prefix[k] : (uint32_t)wb[first + k - plen])) ++k;
        if (k == want) found = s.y;
    }
    return found;
}

// One wave: WordPiece of the word that starts at window position j (the window's words end by `limit`).
__device__ __forceinline__ void wave_word(const WordPieceTables& t, const uint32_t* norm, uint32_t* piece, uint32_t* ph, uint16_t* bo,
                                          uint8_t* wb, uint32_t j, uint32_t limit, uint32_t lane) {
    const uint32_t max_chars = t.max_chars;
    // ---- the word's length in characters, or max_chars + 1 for "longer" ----
    uint32_t len = 1;
    if (cls_of(norm[j]) != kIsolate) {
        for (uint32_t off = 1;; off += 64u) {
            const uint32_t idx = j + off + lane;
            const bool stop = idx >= limit || cls_of(norm[idx]) != kPlain;
            const unsigned long long m = __ballot(stop);
            if (m != 0ull) {
                len = off + (uint32_t)__builtin_ctzll(m);
                break;
            }
            if (off + 64u > max_chars) {
                len = max_chars + 1u;
                break;
            }
        }
    }
    if (len > max_chars) {
        if (lane == 0u) piece[j] = t.unk_id;
        return;
    }
    // ---- prefix hashes and byte offsets of the word's UTF-8: ph[k], bo[k] cover its first k characters ----
    uint32_t carry_h = 0, carry_b = 0;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");   // (the wave's reads of its previous word's prefixes are done)
    __builtin_amdgcn_wave_barrier();
    if (lane == 0u) {
        ph[0] = 0u;
        bo[0] = 0;
    }
    for (uint32_t base = 0; base < len; base += 64u) {
        const uint32_t i = base + lane;
        uint32_t mul = 1u, add = 0u, nb = 0u, cp = 0u;
        if (i < len) {
            cp = norm[j + i] & kValue;
            nb = utf8_len(cp);
            for (uint32_t k = 0; k < nb; ++k) {
                add = add * kWpHashMul + utf8_byte(cp, nb, k);
                mul *= kWpHashMul;
            }
        }
        const uint32_t own = nb;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {   // h -> h * mul + add, composed left to right
            const uint32_t pm = __shfl_up(mul, d), pa = __shfl_up(add, d), pn = __shfl_up(nb, d);
            if (lane >= (uint32_t)d) {
                add = pa * mul + add;
                mul = pm * mul;
                nb += pn;
            }
        }
        const uint32_t h = carry_h * mul + add, b = carry_b + nb;
        if (i < len) {
            ph[i + 1u] = h;
            bo[i + 1u] = (uint16_t)b;
            for (uint32_t k = 0; k < own; ++k) wb[b - own + k] = (uint8_t)utf8_byte(cp, own, k);
        }
        carry_h = __shfl(h, 63);
        carry_b = __shfl(b, 63);
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   // the wave's own LDS writes, before its other lanes read them
    __builtin_amdgcn_wave_barrier();
    // ---- greedy longest match: the lanes are the candidate ends, longest first ----
    uint32_t start = 0, count = 0;
    bool failed = false;
    while (start < len) {   // (every round moves start forward: at most len pieces)
        uint32_t hit_end = 0, hit_id = kNone;
        for (uint32_t r = 0; r * 64u < len - start; ++r) {
            const uint32_t back = r * 64u + lane;
            const bool valid = back < len - start;
            const uint32_t end = len - (valid ? back : 0u);
            const uint32_t id = valid ? lookup_piece(t, ph, bo, wb, start, end) : kNone;
            const unsigned long long m = __ballot(id != kNone);
            if (m != 0ull) {
                const int src = __builtin_ctzll(m);
                hit_end = len - (r * 64u + (uint32_t)src);
                hit_id = __shfl(id, src);
                break;
            }
        }
        if (hit_end == 0u) {
            failed = true;
            break;
        }
        if (lane == 0u) piece[j + count] = hit_id;
        ++count;
        start = hit_end;
    }
    if (failed) {   // the whole word is one [UNK]: the pieces found so far are discarded
        if (lane == 0u) piece[j] = t.unk_id;
        for (uint32_t k = 1u + lane; k < count; k += 64u) piece[j + k] = kNone;
    }
}

__global__ __launch_bounds__(kThreads) void wordpiece_tokenize_kernel(WordPieceTokenizeArgs args) {
    __shared__ uint32_t norm[kCap];
    __shared__ uint32_t piece[kCap];
    __shared__ uint16_t wstart[kCap];
    extern __shared__ uint32_t word_lds[];   // per wave: ph[max_chars + 1] | the word's UTF-8 [4 * max_chars] | bo[max_chars + 2]
    __shared__ uint32_t wsum[kWaves];
    __shared__ uint32_t s_flag, s_words, s_cut, s_text;
    __shared__ uint32_t added_off[kWpMaxAdded + 1];            // the added tokens' contents, out of the per-byte path's global reads
    __shared__ uint8_t added[kWpMaxAdded * kWpMaxAddedBytes];

    __shared__ WordPieceTables lt;   // (both read from LDS where needed: held in scalar registers from the kernel's start they
    __shared__ WordPieceTokenizeArgs a;   // overflowed them)
    const WordPieceTables& t = lt;
    const uint32_t text = blockIdx.x;
    const uint32_t begin = args.offsets[text], end = args.offsets[text + 1];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t out_base = args.piece_base[text], cap = args.piece_base[text + 1] - out_base;
    const uint32_t max_chars = args.max_chars;   // (== t.max_chars)
    uint32_t* const ph = word_lds + wave * wave_lds_words(max_chars);
    uint8_t* const wb = reinterpret_cast<uint8_t*>(ph + max_chars + 1u);
    uint16_t* const bo = reinterpret_cast<uint16_t*>(wb + 4u * max_chars);

    if (tid == 0u) {
        s_flag = 0u;
        s_text = text;
        lt = *args.t;
        a = args;
    }
    __syncthreads();

    const uint32_t n_added = t.added_count < kWpMaxAdded ? t.added_count : kWpMaxAdded;
    for (uint32_t k = tid; k <= n_added; k += kThreads) {
        const uint32_t o = t.added_offsets[k];
        added_off[k] = o < sizeof(added) ? o : (uint32_t)sizeof(added);   // (create() has refused anything longer)
    }
    __syncthreads();
    for (uint32_t k = tid; k < added_off[n_added]; k += kThreads) added[k] = t.added_bytes[k];
    __syncthreads();

    uint32_t fill = 0, pos = begin, emitted = 0;   // the same in every thread
    for (;;) {
        // ---- A: append strides of bytes while one more fits ----
        while (pos < end && fill + kStrideOut <= kCap) {
            uint32_t nout = 0, o0 = 0, o1 = 0, o2 = 0;
            bool flag = false;
            if (tid < end - pos) {
                const uint32_t p = pos + tid;
                const uint32_t left = end - p;
                const uint8_t* __restrict__ bytes = a.text;
                const uint32_t b0 = bytes[p];
                for (uint32_t k = 0; k < n_added; ++k) {   // (at most 32 contents of at most 32 bytes)
                    const uint32_t s = added_off[k], alen = added_off[k + 1u] - s;
                    if (alen > left || added[s] != b0) continue;
                    uint32_t m = 1;
                    while (m < alen && bytes[p + m] == added[s + m]) ++m;
                    flag = flag || m == alen;
                }
                if ((b0 & 0xc0u) != 0x80u) {
                    const uint32_t need = b0 < 0x80u ? 1u : b0 >= 0xf0u ? 4u : b0 >= 0xe0u ? 3u : 2u;
                    if (need <= left) {   // (a sequence the text's end cuts short is dropped: the host has refused such texts)
                        uint32_t cp = need == 1u ? b0 : b0 & (0xffu >> (need + 1u));
                        for (uint32_t i = 1; i < need; ++i) cp = (cp << 6) | (bytes[p + i] & 0x3fu);
                        const uint32_t info = cp < FSGPU_WP_CODE_POINTS ? t.cp_info[cp] : 0u;
                        const uint32_t n = (info >> FSGPU_WP_LEN_SHIFT) & FSGPU_WP_LEN_MASK;
                        flag = flag || (info & FSGPU_WP_HOST) != 0u;
                        if (n == 1u) {
                            const uint32_t c = (info & FSGPU_WP_SPACE) ? kSpace : (info & FSGPU_WP_ISOLATE) ? kIsolate : kPlain;
                            o0 = (info & kValue) | (c << kClsShift);
                            nout = 1;
                        } else if (n == 2u || n == 3u) {
                            const uint32_t at = info & kValue;
                            if (at + n <= t.expansions_len) {
                                o0 = t.expansions[at] & kValue;
                                o1 = t.expansions[at + 1u] & kValue;
                                if (n == 3u) o2 = t.expansions[at + 2u] & kValue;
                                nout = n;
                            }
                        }
                    }
                }
            }
            if (flag) s_flag = 1u;
            uint32_t total;
            const uint32_t at = fill + block_exclusive<kWaves>(nout, lane, wave, wsum, total);
            if (nout > 0u) norm[at] = o0;
            if (nout > 1u) norm[at + 1u] = o1;
            if (nout > 2u) norm[at + 2u] = o2;
            fill += total;
            pos = end - pos > (uint32_t)kThreads ? pos + (uint32_t)kThreads : end;
        }
        __syncthreads();
        if (s_flag != 0u) break;   // (uniform: written before the prefix sum's barriers)
        const bool final = pos >= end;

        // ---- the words this window finishes: all of them, or those before the open last word ----
        uint32_t limit = fill;
        if (!final && fill > 0u && cls_of(norm[fill - 1u]) == kPlain) {
            if (tid == 0u) s_cut = 0u;
            __syncthreads();
            for (uint32_t j = tid; j < fill; j += kThreads)
                if (word_starts(norm, j)) atomicMax(&s_cut, j);
            __syncthreads();
            limit = s_cut;
        }
        if (tid == 0u) s_words = 0u;
        for (uint32_t j = tid; j < limit; j += kThreads) piece[j] = kNone;
        __syncthreads();
        for (uint32_t j = tid; j < limit; j += kThreads)
            if (word_starts(norm, j)) wstart[atomicAdd(&s_words, 1u)] = (uint16_t)j;   // (order is free: a piece's slot is its place)
        __syncthreads();

        // ---- B: one wave per word ----
        const uint32_t words = s_words;
        for (uint32_t w = wave; w < words; w += kWaves) wave_word(t, norm, piece, ph, bo, wb, wstart[w], limit, lane);
        __syncthreads();

        // ---- C: the pieces, in order, into the text's region ----
        for (uint32_t base = 0; base < limit; base += kThreads) {
            const uint32_t j = base + tid;
            const uint32_t id = j < limit ? piece[j] : kNone;
            uint32_t total;
            const uint32_t at = emitted + block_exclusive<kWaves>(id != kNone ? 1u : 0u, lane, wave, wsum, total);
            if (id != kNone && at < cap) a.pieces[out_base + at] = id;
            emitted += total;
        }
        if (final) break;

        // ---- the open word moves to the front (cut at max_chars + 1 characters: it is [UNK] whatever follows) ----
        uint32_t carry = fill - limit;
        if (carry > max_chars + 1u) carry = max_chars + 1u;
        if (limit > 0u)
            for (uint32_t c = 0; c < carry; c += kThreads) {   // (ascending, read then write: a target lies below every later source)
                const uint32_t v = c + tid < carry ? norm[limit + c + tid] : 0u;
                __syncthreads();
                if (c + tid < carry) norm[c + tid] = v;
                __syncthreads();
            }
        fill = carry;
    }

    if (tid == 0u) {
        const bool flagged = s_flag != 0u;
        const uint32_t me = s_text;   // (the block's index, kept in LDS with the arguments)
        a.flagged[me] = flagged ? 1 : 0;
        a.counts[me] = flagged ? 0u : emitted;
    }
}

// pieces of each text that go out and the sequence's length
__device__ __forceinline__ uint32_t sequence_length(const WordPieceAssembleArgs& a, uint32_t i) {
    if (!a.pairs) {
        const uint32_t room = a.piece_base[i + 1u] - a.piece_base[i];
        if (a.flagged[i]) {
            a.keep[i] = 0u;
            a.out_status[i] = 1;
            return 0u;
        }
        uint32_t keep = a.counts[i];
        const uint32_t special = a.add_special ? 2u : 0u;
        if (a.max_length != 0u && keep > a.max_length - special) keep = a.max_length - special;
        if (keep > room) keep = room;
        a.keep[i] = keep;
        a.out_status[i] = 0;
        return keep + special;
    }
    const uint32_t ia = i, ib = a.n + i;
    if (a.flagged[ia] || a.flagged[ib]) {
        a.keep[ia] = a.keep[ib] = 0u;
        a.out_status[i] = 1;
        return 0u;
    }
    uint32_t la = a.counts[ia], lb = a.counts[ib];
    if (a.max_length != 0u) {
        const uint32_t budget = a.max_length - 3u;
        if ((unsigned long long)la + lb > budget) {   // longest_first, in closed form (include/fsgpu.h)
            const bool swap = la > lb;
            uint32_t n1 = swap ? lb : la, n2 = swap ? la : lb;
            n2 = n1 > budget ? n1 : (n1 > budget - n1 ? n1 : budget - n1);
            if ((unsigned long long)n1 + n2 > budget) {
                n1 = budget / 2u;
                n2 = n1 + budget % 2u;
            }
            la = swap ? n2 : n1;
            lb = swap ? n1 : n2;
        }
    }
    const uint32_t room_a = a.piece_base[ia + 1u] - a.piece_base[ia], room_b = a.piece_base[ib + 1u] - a.piece_base[ib];
    if (la > room_a) la = room_a;
    if (lb > room_b) lb = room_b;
    a.keep[ia] = la;
    a.keep[ib] = lb;
    a.out_status[i] = 0;
    return la + lb + 3u;
}

__global__ __launch_bounds__(kOffsetThreads) void wordpiece_offsets_kernel(WordPieceAssembleArgs a) {
    __shared__ uint32_t wsum[kOffsetThreads / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    unsigned long long running = 0ull;
    for (uint32_t base = 0; base < a.n; base += kOffsetThreads) {
        const uint32_t i = base + tid;   // (n is below 2^31: no wrap)
        const uint32_t len = i < a.n ? sequence_length(a, i) : 0u;
        uint32_t total;
        const uint32_t at = block_exclusive<kOffsetThreads / 64>(len, lane, wave, wsum, total);
        if (i < a.n) a.out_offsets[i] = (uint32_t)running + at;   // (the host refuses a total past 2^32 before anything reads these)
        running += total;
    }
    if (tid == 0u) {
        a.out_offsets[a.n] = (uint32_t)running;
        *a.out_total = running;
    }
}

__global__ __launch_bounds__(kThreads) void wordpiece_assemble_kernel(WordPieceAssembleArgs a) {
    const uint32_t i = blockIdx.x;
    const uint32_t o = a.out_offsets[i], len = a.out_offsets[i + 1u] - o;
    if (len == 0u) return;
    if (!a.pairs) {
        const uint32_t sp = a.add_special ? 1u : 0u;
        const uint32_t* __restrict__ src = a.pieces + a.piece_base[i];
        for (uint32_t k = threadIdx.x; k < len; k += kThreads) {
            uint32_t id;
            if (sp && k == 0u) id = a.cls_id;
            else if (sp && k == len - 1u) id = a.sep_id;
            else id = src[k - sp];
            a.out_ids[o + k] = id;
        }
        return;
    }
    const uint32_t ka = a.keep[i];
    const uint32_t* __restrict__ sa = a.pieces + a.piece_base[i];
    const uint32_t* __restrict__ sb = a.pieces + a.piece_base[a.n + i];
    for (uint32_t k = threadIdx.x; k < len; k += kThreads) {
        uint32_t id;
        if (k == 0u) id = a.cls_id;
        else if (k <= ka) id = sa[k - 1u];
        else if (k == ka + 1u || k == len - 1u) id = a.sep_id;
        else id = sb[k - ka - 2u];
        a.out_ids[o + k] = id;
        a.out_type_ids[o + k] = k <= ka + 1u ? 0u : 1u;
    }
}

// The row blocks of the MiniLM short-text forward (bert_docs_pack), from ids that lie on the device: row r of block b is token
// blk_tok[b] + r of the call, or -1 past the block's tokens.
__global__ __launch_bounds__(64) void wordpiece_block_rows_kernel(const int32_t* __restrict__ ids, const uint32_t* __restrict__ blk_tok,
                                                                   int32_t* __restrict__ row_id, uint32_t nblocks) {
    const uint32_t b = blockIdx.x * 2u + (threadIdx.x >> 5), r = threadIdx.x & 31u;
    if (b >= nblocks) return;
    const uint32_t t0 = blk_tok[b], rows = blk_tok[b + 1u] - t0;
    row_id[(size_t)b * 32u + r] = r < rows ? ids[t0 + r] : -1;
}

}  // namespace

hipError_t launch_wordpiece_block_rows(const int32_t* ids_dev, const uint32_t* blk_tok_dev, int32_t* row_id_dev, uint32_t nblocks,
                                       hipStream_t stream) {
    if (nblocks == 0) return hipSuccess;
    hipLaunchKernelGGL(wordpiece_block_rows_kernel, dim3((nblocks + 1) / 2), dim3(64), 0, stream, ids_dev, blk_tok_dev, row_id_dev, nblocks);
    return hipGetLastError();
}

hipError_t launch_wordpiece_tokenize(const WordPieceTokenizeArgs& args, uint32_t texts, hipStream_t stream) {
    if (texts == 0) return hipSuccess;
    if (args.max_chars == 0 || args.max_chars > kWpMaxWordChars) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wordpiece_tokenize_kernel, dim3(texts), dim3(kThreads), kWaves * wave_lds_words(args.max_chars) * 4u, stream, args);
    return hipGetLastError();
}

hipError_t launch_wordpiece_offsets(const WordPieceAssembleArgs& args, hipStream_t stream) {
    if (args.max_length != 0 && args.max_length < (args.pairs ? 3u : (args.add_special ? 2u : 0u))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wordpiece_offsets_kernel, dim3(1), dim3(kOffsetThreads), 0, stream, args);
    return hipGetLastError();
}

hipError_t launch_wordpiece_assemble(const WordPieceAssembleArgs& args, hipStream_t stream) {
    if (args.n == 0) return hipSuccess;
    hipLaunchKernelGGL(wordpiece_assemble_kernel, dim3(args.n), dim3(kThreads), 0, stream, args);
    return hipGetLastError();
}

}  // namespace fsgpu

// fsgpu_lab_api.cpp — the entry points of include/fsgpu_lab.h: stage launchers for kernel-level tests, timers and A/B switches.  None is
// part of the drop-in boundary (fsgpu_api.cpp, include/fsgpu.h); they share its handles and its last-error string (api_internal.hpp).
#include "../../include/fsgpu_lab.h"

#include "api_internal.hpp"
#include "lab_guard.hpp"

#include <algorithm>
#include <cstring>
#include <limits>

using namespace fsgpu::api;

namespace {

namespace lab = fsgpu::lab;

// Device side of the stage entry points: uploads (as they are, as f32, as f16 through launch_bert_to_half, as fragment-order f16 through
// launch_bert_pack_w, a slab with guard rows behind it, a padded bitmap) and outputs that sit between two guard bands (lab_guard.hpp): of 64
// rows for a row-shaped output, of lab::kBand bytes for a byte-sized one.  Everything runs on the null stream.  The first failure sticks;
// every later step is skipped.
struct LabStage {
    static constexpr size_t kGuardRows = 64;
    using Out = lab::Out;
    std::vector<fsgpu::DeviceBuffer> bufs;
    std::vector<Out> outs;
    fsgpu::SearchError e;
    hipError_t he = hipSuccess;
    bool guard_hit = false;

    LabStage() { bufs.reserve(64); }
    ~LabStage() {
        for (fsgpu::DeviceBuffer& b : bufs) b.release();
    }
    // what every lab call that takes a device ordinal does first; FSGPU_OK: go on
    static fsgpu_status open(int32_t device) {
        int count = 0;
        if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(FSGPU_ERR_NO_DEVICE, "no HIP device visible");
        if (device < 0 || device >= count) return fail(FSGPU_ERR_INVALID_CONFIG, "device ordinal out of range");
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_DEVICE, "hipSetDevice failed");
        return FSGPU_OK;
    }
    bool ok() const { return e.ok() && he == hipSuccess; }
    void hip(hipError_t r) {
        if (ok()) he = r;
    }
    void* alloc(size_t bytes) {
        if (!ok()) return nullptr;
        bufs.emplace_back();
        e = bufs.back().reserve(bytes ? bytes : 16);
        return e.ok() ? bufs.back().ptr : nullptr;
    }
    void* raw(const void* src, size_t bytes) {
        void* d = alloc(bytes);
        if (ok()) he = hipMemcpy(d, src, bytes, hipMemcpyHostToDevice);
        return d;
    }
    const float* f32(const float* src, size_t n) { return static_cast<const float*>(raw(src, n * 4)); }
    void* f16(const float* src, size_t n) {
        const float* s = f32(src, n);
        void* d = alloc(n * 2);
        if (ok()) he = fsgpu::launch_bert_to_half(s, d, n, nullptr);
        return d;
    }
    void* packed(const float* w, int N, int K) {
        void* h = f16(w, (size_t)N * K);
        void* d = alloc((size_t)N * K * 2);
        if (ok()) he = fsgpu::launch_bert_pack_w(h, d, N, K, nullptr);
        return d;
    }
    // `body` bytes of src with `tail` bytes of guard rows behind them
    void* with_tail(const void* src, size_t body, size_t tail, lab::Tail t) {
        const std::vector<unsigned char> h = lab::with_guard_tail(src, body, tail, t);
        return raw(h.data(), h.size());
    }
    // a live / allow bitmap of `words` words (two zero words behind the last), or none
    const fsgpu::u64* bitmap(const uint64_t* src, size_t words) {
        if (!src) return nullptr;
        const std::vector<uint64_t> w = lab::padded_bitmap(src, words);
        return static_cast<const fsgpu::u64*>(raw(w.data(), w.size() * 8));
    }
    Out& guarded_out(size_t band, size_t bytes, void* host) {
        Out o;
        o.band = band, o.bytes = bytes, o.host = host;
        o.base = static_cast<unsigned char*>(alloc(o.total()));
        if (ok()) he = hipMemset(o.base, lab::kGuardByte, o.total());
        outs.push_back(o);
        return outs.back();
    }
    // an output of rows x cols elements of elem bytes (1: int8 codes, copied as they are, 2: f16, widened, 4: f32) for the caller's `host`;
    // init: f32 rows the kernel updates in place
    void* out(size_t rows, size_t cols, size_t elem, void* host, const float* init = nullptr) {
        Out& o = guarded_out(kGuardRows * cols * elem, rows * cols * elem, host);
        o.row = cols * elem, o.widen = elem == 2;
        if (ok() && init) he = hipMemcpy(o.ptr(), init, o.bytes, hipMemcpyHostToDevice);
        return ok() ? o.ptr() : nullptr;
    }
    // a byte-sized output for the caller's `host` (none if that is null or bytes is 0), prefilled with the byte `fill`, or (init) with what
    // `host` holds
    void* out_bytes(size_t bytes, int fill, void* host, bool init = false) {
        if (bytes == 0 || !host) return nullptr;
        Out& o = guarded_out(lab::kBand, bytes, host);
        if (ok()) he = init ? hipMemcpy(o.ptr(), host, bytes, hipMemcpyHostToDevice) : hipMemset(o.ptr(), fill, bytes);
        return ok() ? o.ptr() : nullptr;
    }
    // an input workspace of `slabs` x 32 rows of f32 (f16: rounded on the device) whose rows m..31 hold NaN: host [slabs][m][cols]
    void* workspace(const float* src, size_t slabs, size_t m, size_t cols, bool half) {
        std::vector<float> h(slabs * 32 * cols, std::numeric_limits<float>::quiet_NaN());
        for (size_t sl = 0; sl < slabs; ++sl) std::memcpy(h.data() + sl * 32 * cols, src + sl * m * cols, m * cols * 4);
        return half ? f16(h.data(), h.size()) : const_cast<float*>(f32(h.data(), h.size()));
    }
    // the four-slab output: [slabs][32][cols] f32, all of it guard bytes beforehand; rows m..31 of each slab must keep them
    void* out_slabs(size_t slabs, size_t m, size_t cols, float* host) {
        void* p = out(slabs * 32, cols, 4, host);
        outs.back().slab_rows = m;
        return p;
    }
    // a buffer the launch is handed (or not) and must not write: guard bytes throughout, checked whole
    void* out_untouched(size_t rows, size_t cols, size_t elem) {
        void* p = out(rows, cols, elem, nullptr);
        outs.back().untouched = true, outs.back().widen = false;
        return p;
    }
    void collect() {
        hip(hipStreamSynchronize(nullptr));
        for (const Out& o : outs) {
            if (!ok()) return;
            std::vector<unsigned char> h(o.total());
            he = hipMemcpy(h.data(), o.base, h.size(), hipMemcpyDeviceToHost);
            if (!ok()) return;
            if (lab::collect_out(o, h.data())) guard_hit = true;
            if (o.widen) {
                const _Float16* s = reinterpret_cast<const _Float16*>(h.data() + o.band);
                for (size_t i = 0; i < o.bytes / 2; ++i) static_cast<float*>(o.host)[i] = (float)s[i];
            }
        }
    }
    // collect(), then what the entry point returns: an allocation failure, (refused given) a launcher's hipErrorInvalidValue, any other HIP
    // error, a touched guard byte
    fsgpu_status status(const char* guard_message, const char* refused = nullptr) {
        collect();
        if (!e.ok()) return finish(e);
        if (refused && he == hipErrorInvalidValue) return fail(FSGPU_ERR_INVALID_CONFIG, refused);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        if (guard_hit) return fail(FSGPU_ERR_DEVICE, guard_message);
        return FSGPU_OK;
    }
};

// offsets [n_docs + 1] from 0 to m, non-decreasing; the longest document (embed_batch's max_seq)
bool lab_offsets(const uint32_t* offsets, uint32_t n_docs, uint32_t m, uint32_t* max_seq, uint32_t* min_seq) {
    if (!offsets || n_docs == 0 || n_docs > (1u << 20) || offsets[0] != 0 || offsets[n_docs] != m) return false;
    *max_seq = 0;
    *min_seq = ~0u;
    for (uint32_t i = 0; i < n_docs; ++i) {
        if (offsets[i + 1] < offsets[i]) return false;
        const uint32_t len = offsets[i + 1] - offsets[i];
        *max_seq = std::max(*max_seq, len);
        *min_seq = std::min(*min_seq, len);
    }
    return true;
}

// What fsgpu_lab_scan_stage derives from its arguments once they have passed: queries per group, groups, row pitch, output sizes.
struct ScanStageGeom {
    uint32_t group_q = 0, groups = 1;
    bool sample = false, lists = false, counts = false;
    size_t pitch = 0, cand_n = 0, count_n = 0, spill_n = 0, dense_n = 0;
};

fsgpu_status scan_stage_check(const fsgpu_lab_scan_stage_args& a, ScanStageGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    ScanStageGeom g;
    if (a.kernel > FSGPU_LAB_SCAN_PREPARE) return bad("scan stage: unknown kernel");
    if (a.elem_bytes != 1 && a.elem_bytes != 2) return bad("scan stage: elem_bytes must be 1 or 2");
    if (a.kernel == FSGPU_LAB_SCAN_PREPARE) {
        if (a.dim == 0 || a.dim > 4096) return bad("scan stage: prepare takes dim in 1..=4096");
        if (a.nq_pad == 0 || a.nq_pad > 4096 || a.nq > a.nq_pad) return bad("scan stage: prepare takes nq <= nq_pad in 1..=4096");
        if (a.elem_bytes == 1 && a.bits != 8 && a.bits != 4) return bad("scan stage: the int8 prepare takes bits 8 or 4");
        if ((a.nq && !a.queries_f32) || !a.prepared || !a.delta) return null("scan stage: prepare needs queries_f32, prepared and delta");
        if (geom) *geom = g;
        return FSGPU_OK;
    }
    const int dim = (int)a.dim, eb = (int)a.elem_bytes;
    if (a.nrows == 0 || a.nrows > (1u << 24)) return bad("scan stage: nrows must be in 1..=2^24");
    if (a.grid == 0 || a.grid > 4096 || a.groups > 8) return bad("scan stage: grid must be in 1..=4096 and groups at most 8");
    if (a.spill_cap > (1u << 20) || a.group_count > (1u << 16) || a.side_by_side > 1 || a.reverse > 1 || a.want_counts > 1)
        return bad("scan stage: spill_cap, group_count or a flag out of range");
    g.groups = a.groups ? a.groups : 1;
    if (a.kernel == FSGPU_LAB_SCAN_LDS) {
        if (!fsgpu::scan_mfma_supported(dim)) return bad("scan stage: scan_mfma_supported refuses the dimension");
        if (a.variant > 5 || !fsgpu::scan_mfma_shape_built((int)a.variant) || (a.variant == 4 && eb != 1))
            return bad("scan stage: the shape is not compiled into this build");
        if (a.stage > 2) return bad("scan stage: the LDS-query kernel has stages 0, 1 and 2");
        if (a.want_counts || a.side_by_side) return bad("scan stage: list lengths and side-by-side groups are the register-query kernel's");
        if (a.stage != 0 && (a.slots == 0 || (int)a.slots > fsgpu::scan_mfma_max_slots((int)a.variant))) return bad("scan stage: slots beyond scan_mfma_max_slots");
        g.group_q = (uint32_t)fsgpu::scan_mfma_query_tiles((int)a.variant) * 16;
        g.sample = a.stage < 2;
        if (a.group_stride == 0) return bad("scan stage: group_stride must be at least 1");
    } else {
        if (!fsgpu::scan_wide_supported(dim, eb)) return bad("scan stage: scan_wide_supported refuses the row length");
        if (a.variant < 2 || (int)a.variant > fsgpu::scan_wide_max_query_tiles(dim, eb)) return bad("scan stage: query tiles beyond scan_wide_max_query_tiles");
        if (a.stage < 1 || a.stage > 3) return bad("scan stage: the register-query kernel has stages 1, 2 and 3");
        if (a.stage == 3 && (eb != 1 || !fsgpu::scan_wide_group_maxima_supported(dim, (int)a.variant)))
            return bad("scan stage: scan_wide_group_maxima_supported refuses the shape");
        if (a.stage == 3 && a.want_counts) return bad("scan stage: the group-maxima stage writes no lists");
        if (a.stage != 3 && (a.slots == 0 || a.slots > fsgpu::kWideSlots)) return bad("scan stage: slots beyond kWideSlots");
        g.group_q = 128 * a.variant;
        g.sample = a.stage != 2;
        if (a.stage == 2 && a.group_count != 0) return bad("scan stage: the register-query main pass visits every row (group_count must be 0)");
        // (the kernel's list offsets are 32-bit byte offsets inside a group's lists)
        if ((uint64_t)g.group_q * a.grid * (a.stage == 3 ? 4 : a.slots) * 8 > 0xffffffffull) return bad("scan stage: a group's lists exceed 4 GB");
    }
    if (g.sample) {
        if (a.group_count == 0 || a.group_stride == 0) return bad("scan stage: a sample stage needs group_count and group_stride");
        if ((uint64_t)(a.group_count - 1) * a.group_stride * 64 >= a.nrows) return bad("scan stage: a sample group begins past the last row");
    }
    if (a.nq_pad != g.groups * g.group_q) return bad("scan stage: nq_pad must be groups x the kernel's query group");
    g.pitch = a.row_stride ? a.row_stride : (size_t)dim * eb;
    if (g.pitch < (size_t)dim * eb || (g.pitch & 15) || g.pitch > (1u << 16)) return bad("scan stage: row_stride must be a multiple of 16 bytes that holds a row");
    if ((uint64_t)a.nrows * g.pitch > (1ull << 31)) return bad("scan stage: the slab exceeds 2 GB");
    const bool gmax = a.kernel == FSGPU_LAB_SCAN_REG && a.stage == 3;
    const bool dense = a.kernel == FSGPU_LAB_SCAN_LDS && a.stage == 0;
    g.lists = !dense && !gmax;
    g.counts = a.want_counts != 0;
    g.cand_n = dense ? 0 : (size_t)a.nq_pad * a.grid * (gmax ? 4 : a.slots);
    g.count_n = g.counts ? (size_t)a.nq_pad * a.grid : 0;
    g.spill_n = g.lists ? (size_t)a.nq_pad * a.spill_cap : 0;
    g.dense_n = dense ? (size_t)a.nq_pad * a.group_count * 64 : 0;
    if ((g.cand_n | g.dense_n) > (1ull << 28)) return bad("scan stage: an output exceeds 2 GB");
    if (!a.slab || !a.queries) return null("scan stage: slab or queries is null");
    if (!dense && !gmax && !a.tau) return null("scan stage: tau is null");
    if (dense ? !a.dense : !a.cand) return null("scan stage: the stage's output is null");
    if (g.lists && (!a.spill_count || !a.overflow || (a.spill_cap && !a.spill))) return null("scan stage: spill, spill_count or overflow is null");
    if (g.counts && !a.cand_count) return null("scan stage: cand_count is null");
    if (geom) *geom = g;
    return FSGPU_OK;
}

// What fsgpu_lab_select derives from its arguments once they have passed: array sizes in elements.
struct SelectGeom {
    size_t lists_n = 0, exact_n = 0, counts_n = 0, query_rows = 0, query_pitch = 0, slab_pitch = 0, bitmap_words = 0;
    bool finish = false;
};

fsgpu_status select_check(const fsgpu_lab_select_args& a, SelectGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    SelectGeom g;
    if (a.kernel > FSGPU_LAB_TWO_PASS_MERGE) return bad("select: unknown kernel");
    if (a.kernel != FSGPU_LAB_LIST_CUT && (a.nq == 0 || a.nq > 4096)) return bad("select: nq must be in 1..=4096");
    if (a.valid_queries > a.nq) return bad("select: valid_queries beyond nq");
    if (a.dim > 4096 || a.nrows > (1u << 22) || a.spill_cap > (1u << 20) || a.extra_len > (1u << 20) || a.out_stride > 4096 || a.cand_out_stride > 4096)
        return bad("select: dim, nrows, spill_cap, extra_len or an output stride out of range");
    if (a.reset_spill > 1 || a.big_pool > 2 || a.hreduce < 0 || a.hreduce > 2) return bad("select: a flag out of range");
    // the slab and the queries of a re-score (SELECT's finish, the anchored SELECT_GROUPS)
    auto rescore_geom = [&](bool strided) -> fsgpu_status {
        const size_t elem = a.slab_f32 ? 4 : 2;
        g.slab_pitch = strided && a.row_stride ? a.row_stride : (size_t)a.dim * elem;
        if (a.dim == 0 || a.nrows == 0) return bad("select: a re-score needs dim and nrows");
        if (g.slab_pitch < (size_t)a.dim * elem || (g.slab_pitch & 15) || g.slab_pitch > (1u << 16)) return bad("select: row_stride must be a multiple of 16 bytes that holds a row");
        if ((uint64_t)a.nrows * g.slab_pitch > (1ull << 30)) return bad("select: the slab exceeds 1 GB");
        g.query_pitch = a.query_stride ? a.query_stride : a.dim;
        if (g.query_pitch < a.dim) return bad("select: query_stride below dim");
        g.query_rows = a.valid_queries ? a.valid_queries : a.nq;
        g.bitmap_words = ((size_t)a.nrows + 63) / 64;
        if (!a.queries) return null("select: queries is null");
        return FSGPU_OK;
    };
    if (a.kernel == FSGPU_LAB_SELECT) {
        fsgpu::SelectArgs s{};
        s.nlists = a.nlists, s.list_len = a.list_len, s.k = a.k, s.k_out = a.k_out, s.dim = a.dim, s.row_stride = a.row_stride, s.slab_f32 = a.slab_f32;
        s.delta = a.delta, s.slab = a.slab;
        if (!a.delta) return null("select: delta is null");
        if (!fsgpu::select_args_ok(s)) return bad("select: launch_select refuses the arguments");
        const uint64_t need = a.nlists && a.list_len ? (uint64_t)(a.nlists - 1) * a.l_stride + a.list_len : 0;
        if (a.l_stride < a.list_len || a.q_stride < need || (uint64_t)a.nq * a.q_stride > (1ull << 25)) return bad("select: q_stride / l_stride do not hold the lists, or they exceed 2^25 entries");
        if ((uint64_t)a.nlists * a.list_len + a.extra_len + a.spill_cap > (1u << 22)) return bad("select: more than 2^22 entries per query");
        g.lists_n = (size_t)a.nq * a.q_stride;
        g.counts_n = (size_t)a.nq * a.nlists;
        if (need && !a.lists) return null("select: lists is null");
        if (a.extra_len && !a.extra) return null("select: extra is null");
        if (a.spill && !a.spill_count) return null("select: spill without spill_count");
        if (a.reset_spill && !a.spill_count) return null("select: reset_spill without spill_count");
        if (a.big_pool && !a.pool_flag) return null("select: the big-pool forms need pool_flag");
        g.finish = a.slab != nullptr;
        if (g.finish) {
            if (const fsgpu_status st = rescore_geom(true); st != FSGPU_OK) return st;
            if (a.out_stride < a.k_out) return bad("select: out_stride below k_out");
            if ((a.cand_approx_out || a.cand_exact_out) && a.cand_out_stride < a.k) return bad("select: cand_out_stride below k");
        } else if (a.big_pool || a.anchor_unit || a.out_rows || a.out_scores || a.out_packed || a.out_counts || a.cand_approx_out || a.cand_exact_out) {
            return bad("select: a finish field without a slab");
        }
    } else if (a.kernel == FSGPU_LAB_SELECT_GROUPS) {
        fsgpu::GroupSelectArgs s{};
        s.nentries = a.nentries, s.k = a.k, s.dim = a.dim, s.rank_only = a.rank_only;
        s.delta = a.delta, s.tau_out = a.tau_out, s.anchor_unit = a.anchor_unit, s.slab = a.slab;
        if (!a.delta || !a.tau_out) return null("select: delta or tau_out is null");
        if (!a.rank_only && (!a.anchor_unit || !a.slab)) return null("select: the anchored form needs anchor_unit and slab");
        if (!fsgpu::select_groups_args_ok(s)) return bad("select: launch_select_groups refuses the arguments");
        if (!a.lists) return null("select: lists is null");
        if (a.reset_spill && !a.spill_count) return null("select: reset_spill without spill_count");
        g.lists_n = (size_t)a.nq * a.nentries;
        g.finish = !a.rank_only;
        if (g.finish)
            if (const fsgpu_status st = rescore_geom(false); st != FSGPU_OK) return st;
    } else if (a.kernel == FSGPU_LAB_LIST_CUT) {
        if (!fsgpu::list_cut_args_ok(a.nlists, a.list_len)) return bad("select: launch_list_cut refuses the arguments");
        if ((uint64_t)a.nlists * a.list_len > (1ull << 25)) return bad("select: the lists exceed 2^25 entries");
        g.lists_n = (size_t)a.nlists * a.list_len;
        if ((g.lists_n && !a.lists) || !a.tau_out) return null("select: lists or tau_out is null");
    } else {
        if (!fsgpu::two_pass_merge_args_ok(a.nshards, a.cc, a.k)) return bad("select: launch_two_pass_merge refuses the arguments");
        if (a.nshards == 0 || a.shard_pitch < (uint64_t)a.nq * a.cc || (uint64_t)a.nshards * a.shard_pitch > (1ull << 25)) return bad("select: shard_pitch does not hold nq x cc entries, or the lists exceed 2^25");
        g.lists_n = g.exact_n = (size_t)a.nshards * a.shard_pitch;
        if (!a.lists || !a.exact_lists) return null("select: lists or exact_lists is null");
    }
    if (geom) *geom = g;
    return FSGPU_OK;
}

// What fsgpu_lab_lone_stage derives from its arguments once they have passed: sizes in bytes / elements.
struct LoneGeom {
    size_t row_bytes = 0, slab_pitch = 0, query_bytes = 0, bitmap_words = 0, lists_n = 0;
};

fsgpu_status lone_stage_check(const fsgpu_lab_lone_stage_args& a, LoneGeom* geom) {
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    auto null = [](const char* what) { return fail(FSGPU_ERR_NULL_ARGUMENT, what); };
    LoneGeom g;
    if (a.kind > FSGPU_LAB_LONE_MERGE) return bad("lone: unknown kind");
    if (a.kind == FSGPU_LAB_LONE_MERGE) {
        if (a.nq == 0 || a.nq > 4096) return bad("lone: nq must be in 1..=4096");
        if (a.nlists == 0 || a.list_len == 0) return bad("lone: a merge needs nlists and list_len");
        if (a.k == 0 || a.k > 256) return bad("lone: k must be in 1..=256");
        if (a.out_stride < a.k || a.out_stride > 4096) return bad("lone: out_stride below k, or above 4096");
        if (a.lists_sorted > 1) return bad("lone: a flag out of range");
        if ((uint64_t)a.nlists * a.list_len > (1u << 22)) return bad("lone: more than 2^22 entries per query");
        const uint64_t need = (uint64_t)(a.nlists - 1) * a.l_stride + a.list_len;
        if (a.l_stride < a.list_len || a.q_stride < need || (uint64_t)a.nq * a.q_stride > (1ull << 25))
            return bad("lone: q_stride / l_stride do not hold the lists, or they exceed 2^25 entries");
        g.lists_n = (size_t)a.nq * a.q_stride;
        if (!a.lists) return null("lone: lists is null");
        if (geom) *geom = g;
        return FSGPU_OK;
    }
    const int nq = (int)a.nq, tier = (int)a.tier, dim = (int)a.dim;
    if (a.tier != 64 && a.tier != 256) return bad("lone: tier must be 64 or 256");
    if (a.k == 0 || a.k > a.tier) return bad("lone: k must be in 1..=tier");
    if (a.grid == 0 || a.grid > 4096) return bad("lone: grid must be in 1..=4096");
    if (a.nrows == 0 || a.nrows > (1u << 22)) return bad("lone: nrows must be in 1..=2^22");
    if (a.dim == 0 || a.dim > 4096 || (a.dim & 7)) return bad("lone: dim must be a multiple of 8 up to 4096");
    if (a.hreduce < 0 || a.hreduce > 2 || a.force_runtime_dim > 1 || a.plain_loads > 1) return bad("lone: a flag out of range");
    if (a.kind != FSGPU_LAB_LONE_F16 && (a.force_runtime_dim || a.plain_loads)) return bad("lone: force_runtime_dim / plain_loads are launch_scan_topk's");
    bool strided_ok = false;
    switch (a.kind) {
        case FSGPU_LAB_LONE_F16:
            if (nq != 1 && nq != 2 && nq != 4) return bad("lone: launch_scan_topk takes 1, 2 or 4 queries per pass");
            if (fsgpu::scan_lds_bytes(dim, nq, tier) > 160 * 1024) return bad("lone: the queries and lists exceed the LDS");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)nq * dim * 4, strided_ok = true;
            break;
        case FSGPU_LAB_LONE_F16_HOST_QUERY:
            if (nq != 1) return bad("lone: the host-query form takes one query");
            if (!fsgpu::scan_kernarg_query_supported(dim, tier)) return bad("lone: scan_kernarg_query_supported refuses the shape");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)dim * 4, strided_ok = true;
            break;
        case FSGPU_LAB_LONE_F16_MQ:
            if (!fsgpu::scan_mq_supported(dim, nq, tier)) return bad("lone: scan_mq_supported refuses the shape");
            g.row_bytes = (size_t)dim * 2, g.query_bytes = (size_t)nq * dim * 4;
            break;
        case FSGPU_LAB_LONE_I8:
            if (nq != 1) return bad("lone: the int8 scan takes one query");
            if (!fsgpu::scan_i8_fused_supported(dim, tier)) return bad("lone: scan_i8_fused_supported refuses the shape");
            g.row_bytes = g.query_bytes = (size_t)dim;
            break;
        case FSGPU_LAB_LONE_I4:
            if (nq != 1) return bad("lone: the 4-bit scan takes one query");
            if (!fsgpu::scan_4bit_fused_supported(dim, tier)) return bad("lone: scan_4bit_fused_supported refuses the shape");
            g.row_bytes = g.query_bytes = (size_t)dim / 2;
            break;
        default:
            if (nq != 1 && nq != 2 && nq != 4) return bad("lone: launch_scan_topk_f32 takes 1, 2 or 4 queries per pass");
            if ((size_t)nq * dim * 4 > (size_t)96 * 1024 || fsgpu::scan_lds_bytes(dim, nq, tier) > 160 * 1024)
                return bad("lone: the queries and lists exceed the LDS");
            g.row_bytes = (size_t)dim * 4, g.query_bytes = (size_t)nq * dim * 4, strided_ok = true;
            break;
    }
    g.slab_pitch = a.row_stride ? a.row_stride : g.row_bytes;
    if (g.slab_pitch < g.row_bytes || (g.slab_pitch & 15) || g.slab_pitch > (1u << 16)) return bad("lone: row_stride must be a multiple of 16 bytes that holds a row");
    if (!strided_ok && g.slab_pitch != g.row_bytes) return bad("lone: this kernel reads dense rows only");
    if ((uint64_t)a.nrows * g.slab_pitch > (1ull << 30)) return bad("lone: the slab exceeds 1 GB");
    g.bitmap_words = ((size_t)a.nrows + 63) / 64;
    if ((a.live || a.allow) && a.bitmap_words < g.bitmap_words) return bad("lone: a bitmap shorter than the rows");
    if (!a.slab || !a.queries || !a.partial) return null("lone: slab, queries or partial is null");
    if (geom) *geom = g;
    return FSGPU_OK;
}

}  // namespace

extern "C" {

const char* fsgpu_last_main_pass_kernel(void) { return fsgpu::last_main_pass_kernel(); }

fsgpu_status fsgpu_index_set_profiling(fsgpu_index* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.profiling = enabled != 0;
    idx->impl.profile_period = enabled > 1 ? enabled : 1;
    idx->impl.profile_tick_ = 0;
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_scan_time(fsgpu_index* idx, double* total_ms, uint64_t* launches, int32_t reset) {
    if (!idx || !total_ms || !launches) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.scan_time(total_ms, launches, nullptr, reset != 0));
    });
}

fsgpu_status fsgpu_index_scan_stats(fsgpu_index* idx, double* total_ms, uint64_t* launches, uint64_t* rows, int32_t reset) {
    if (!idx || !total_ms || !launches || !rows) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.scan_time(total_ms, launches, rows, reset != 0));
    });
}

fsgpu_status fsgpu_index_filter_stats(fsgpu_index* idx, uint64_t* gathered, uint64_t* scanned) {
    if (!idx || !gathered || !scanned) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);   // no search is running on any lane
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    *gathered = idx->impl.filter_gathered;
    *scanned = idx->impl.filter_scanned;
    for (size_t i = 0; i < idx->impl.replica_count(); ++i) {
        *gathered += idx->impl.replica(i)->filter_gathered;
        *scanned += idx->impl.replica(i)->filter_scanned;
    }
    return FSGPU_OK;
}

fsgpu_status fsgpu_index_set_variant(fsgpu_index* idx, int32_t variant) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::unique_lock<std::shared_mutex> state(idx->state_mu);
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.variant = variant;
    idx->impl.sync_replicas();
    return FSGPU_OK;
}


fsgpu_status fsgpu_lab_multi_filter_plan(uint64_t nrows, const uint64_t* allowed_per_filter, uint32_t nfilters, const int32_t* filter_of_query,
                                         uint32_t nq, int32_t* out_group_of_query, int32_t* out_path_of_group, uint32_t* out_ngroups) {
    if ((nfilters && !allowed_per_filter) || (nq && (!filter_of_query || !out_group_of_query || !out_path_of_group)) || !out_ngroups)
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        return finish(fsgpu::multi_filter_plan(nrows, allowed_per_filter, nfilters, filter_of_query, nq, out_group_of_query, out_path_of_group,
                                               nullptr, out_ngroups));
    });
}

fsgpu_status fsgpu_lab_index_wal_scores(fsgpu_index* idx, const float* queries, uint32_t nq, float* out) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    if (nq && (!queries || !out)) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.lab_wal_scores(queries, nq, out));
    });
}

fsgpu_status fsgpu_lab_index_set_compact_launch_rows(fsgpu_index* idx, uint32_t rows) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.compact_launch_rows = rows;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_set_compact_nt_stores(fsgpu_index* idx, int32_t enabled) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    idx->impl.compact_nt_stores = enabled != 0;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_last_rewrite(fsgpu_index* idx, double* out_ms5, uint64_t* out_counts3) {
    if (!idx || !out_ms5 || !out_counts3) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    const fsgpu::VectorIndex::RewriteTimes& t = idx->impl.last_rewrite;
    out_ms5[0] = t.plan_ms, out_ms5[1] = t.kernel_ms, out_ms5[2] = t.tables_ms, out_ms5[3] = t.file_ms, out_ms5[4] = t.rebuild_ms;
    out_counts3[0] = t.runs, out_counts3[1] = t.launches, out_counts3[2] = t.dst_bytes;
    return FSGPU_OK;
}
fsgpu_status fsgpu_lab_index_attach_synthetic_doc_ids(fsgpu_index* idx) {
    if (!idx) return fail(FSGPU_ERR_NULL_ARGUMENT, "index is null");
    return guarded([&]() -> fsgpu_status {
        std::unique_lock<std::shared_mutex> state(idx->state_mu);
        std::lock_guard<std::mutex> lock(idx->impl.mutex());
        return finish(idx->impl.lab_attach_synthetic_doc_ids());
    });
}
fsgpu_status fsgpu_lab_device_copy_ms(int32_t device, uint64_t bytes, uint32_t reps, double* out_ms) {
    if (!out_ms && reps) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        if (hipSetDevice(device) != hipSuccess) return fail(FSGPU_ERR_NO_DEVICE, "hipSetDevice failed");
        fsgpu::DeviceBuffer a, b;
        fsgpu::SearchError e = a.reserve((size_t)bytes);
        if (e.ok()) e = b.reserve((size_t)bytes);
        hipEvent_t e0 = nullptr, e1 = nullptr;
        hipError_t he = hipSuccess;
        if (e.ok()) he = hipMemset(a.ptr, 1, (size_t)bytes);
        if (e.ok() && he == hipSuccess) he = hipEventCreate(&e0);
        if (e.ok() && he == hipSuccess) he = hipEventCreate(&e1);
        for (uint32_t r = 0; e.ok() && he == hipSuccess && r < reps; ++r) {
            he = hipEventRecord(e0, nullptr);
            if (he == hipSuccess) he = hipMemcpyAsync(b.ptr, a.ptr, (size_t)bytes, hipMemcpyDeviceToDevice, nullptr);
            if (he == hipSuccess) he = hipEventRecord(e1, nullptr);
            if (he == hipSuccess) he = hipEventSynchronize(e1);
            float ms = 0.f;
            if (he == hipSuccess) he = hipEventElapsedTime(&ms, e0, e1);
            out_ms[r] = ms;
        }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        a.release();
        b.release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_index_query_hubness_topk(fsgpu_index* idx, const float* queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                                float* out, float* out_topk) {
    if (idx && idx->impl.record_count() && !out_topk) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_topk is null");
    return index_query_hubness(idx, queries, nq, query_dim, kq, out, out_topk);
}

fsgpu_status fsgpu_lab_index_knn_build_stats(fsgpu_index* idx, uint64_t* out4) {
    if (!idx || !out4) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    std::lock_guard<std::mutex> lock(idx->impl.mutex());
    const fsgpu::VectorIndex::KnnBuildStats& st = idx->impl.last_knn_build;
    out4[0] = st.steps, out4[1] = st.sources, out4[2] = st.fallbacks, out4[3] = st.late_answers;
    return FSGPU_OK;
}

fsgpu_status fsgpu_bench_fixture_device(int32_t device, uint64_t first, uint64_t n, uint32_t dim, uint32_t clusters, float noise,
                                        uint64_t seed_base, int32_t as_f16, void* out_dev, void* hip_stream) {
    if (n && !out_dev) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_dev is null");
    if (dim == 0 || clusters == 0) return fail(FSGPU_ERR_INVALID_CONFIG, "dim and clusters must be positive");
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        fsgpu::DeviceBuffer cent;
        fsgpu::SearchError e = cent.reserve((size_t)clusters * dim * 4);
        if (!e.ok()) return finish(e);
        hipStream_t st = static_cast<hipStream_t>(hip_stream);
        hipError_t he = fsgpu::launch_bench_fixture(first, n, dim, clusters, noise, seed_base, static_cast<float*>(cent.ptr),
                                                    as_f16 ? static_cast<unsigned short*>(out_dev) : nullptr,
                                                    as_f16 ? nullptr : static_cast<float*>(out_dev), st);
        if (he == hipSuccess) he = hipStreamSynchronize(st);
        cent.release();
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_sort_keys_desc(int32_t device, const uint64_t* keys, uint64_t n, uint64_t varying_bits, uint64_t* out_sorted) {
    if (n && (!keys || !out_sorted)) return fail(FSGPU_ERR_NULL_ARGUMENT, "keys / out_sorted is null");
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        if (n == 0) return FSGPU_OK;
        fsgpu::DeviceBuffer in, out, tmp;
        size_t tmp_bytes = 0;
        (void)fsgpu::sort_keys_desc_temp_bytes(n, &tmp_bytes);
        fsgpu::SearchError e = in.reserve(n * 8);
        if (e.ok()) e = out.reserve(n * 8);
        if (e.ok()) e = tmp.reserve(tmp_bytes);
        hipError_t he = hipSuccess;
        if (e.ok()) {
            he = hipMemcpy(in.ptr, keys, n * 8, hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = fsgpu::sort_keys_desc(tmp.ptr, tmp.bytes, static_cast<const fsgpu::u64*>(in.ptr), static_cast<fsgpu::u64*>(out.ptr), n, nullptr, varying_bits);
            if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
            if (he == hipSuccess) he = hipMemcpy(out_sorted, out.ptr, n * 8, hipMemcpyDeviceToHost);
        }
        in.release();
        out.release();
        tmp.release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_linear_int8_dynamic(int32_t device, const float* x, const float* w, const float* bias, uint32_t m, uint32_t n,
                                           uint32_t k, float* y) {
    if ((m && (!x || !y)) || !w || !bias) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (!fsgpu::bert_i8_gemm_supported((int)n, (int)k) || n > (1u << 20) || k > (1u << 20))
        return fail(FSGPU_ERR_INVALID_CONFIG, "int8 linear: K and N must be multiples of 64");
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        if (m == 0) return FSGPU_OK;
        fsgpu::DeviceBuffer dx, dw, db, dy, qx, sx, wp, sw;
        fsgpu::SearchError e = dx.reserve((size_t)m * k * 4);
        if (e.ok()) e = dw.reserve((size_t)n * k * 4);
        if (e.ok()) e = db.reserve((size_t)n * 4);
        if (e.ok()) e = dy.reserve((size_t)m * n * 4);
        if (e.ok()) e = qx.reserve((size_t)m * k);
        if (e.ok()) e = sx.reserve((size_t)m * 4);
        if (e.ok()) e = wp.reserve(fsgpu::bert_i8_packed_bytes((int)n, (int)k));
        if (e.ok()) e = sw.reserve((size_t)n * 4);
        hipError_t he = hipSuccess;
        if (e.ok()) {
            he = hipMemcpy(dx.ptr, x, (size_t)m * k * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(dw.ptr, w, (size_t)n * k * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess) he = hipMemcpy(db.ptr, bias, (size_t)n * 4, hipMemcpyHostToDevice);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_pack_w(static_cast<const float*>(dw.ptr), wp.ptr, static_cast<float*>(sw.ptr), (int)n, (int)k, nullptr);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_quant_rows(static_cast<const float*>(dx.ptr), qx.ptr, static_cast<float*>(sx.ptr), (int)m, (int)k, nullptr);
            if (he == hipSuccess)
                he = fsgpu::launch_bert_i8_gemm(qx.ptr, static_cast<const float*>(sx.ptr), wp.ptr, static_cast<const float*>(sw.ptr),
                                                static_cast<const float*>(db.ptr), static_cast<float*>(dy.ptr), (int)m, (int)n, (int)k, false, nullptr);
            if (he == hipSuccess) he = hipStreamSynchronize(nullptr);
            if (he == hipSuccess) he = hipMemcpy(y, dy.ptr, (size_t)m * n * 4, hipMemcpyDeviceToHost);
        }
        for (fsgpu::DeviceBuffer* b : {&dx, &dw, &db, &dy, &qx, &sx, &wp, &sw}) b->release();
        if (!e.ok()) return finish(e);
        if (he != hipSuccess) return fail(FSGPU_ERR_DEVICE, hipGetErrorString(he));
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_bert_stage(int32_t device, const fsgpu_lab_bert_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_stage_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    const int M = (int)a.m, N = (int)a.n, K = (int)a.k, H = (int)a.hidden, I = (int)a.inter;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (a.m == 0 || a.m > (1u << 20)) return bad("bert stage: m must be in 1..=2^20");
    if (st > FSGPU_LAB_BERT_CLS_HEAD || form > 2) return bad("bert stage: unknown stage or form");
    static const int n_in[] = {1, 3, 6, 12, 5, 1, 5};
    const int need = n_in[st] + ((st == FSGPU_LAB_BERT_ATTENTION && form == 2) ? 1 : 0);
    for (int i = 0; i < need; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: missing input");
    if (!a.out0) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: out0 is null");
    const bool two_outs = st == FSGPU_LAB_BERT_LINEAR_LN || st == FSGPU_LAB_BERT_POST_ATTN || st == FSGPU_LAB_BERT_EMBED_LN ||
                          st == FSGPU_LAB_BERT_CLS_HEAD || (st == FSGPU_LAB_BERT_ATTENTION && form == 2);
    if (two_outs && !a.out1) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert stage: out1 is null");
    // the encoder's own shape rule (NativeEmbedder::init); the linear stage has no hidden, the head has the reranker's rule
    if (st == FSGPU_LAB_BERT_CLS_HEAD) {
        if (form != 0 || !fsgpu::bert_rerank_supported(H)) return bad("bert stage: the head takes a hidden that is a multiple of 64 and <= 1024");
    } else if (st != FSGPU_LAB_BERT_LINEAR && (H <= 0 || H % 128 != 0 || H > 1024)) {
        return bad("bert stage: hidden must be a multiple of 128 and <= 1024");
    }
    uint32_t max_seq = 0, min_seq = 0;
    switch (st) {
        case FSGPU_LAB_BERT_ATTENTION:
            if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq) || max_seq > 512) return bad("bert stage: offsets must run from 0 to m in documents of at most 512 tokens");
            if (form == 2 && (min_seq == 0 || !fsgpu::bert_rerank_supported(H))) return bad("bert stage: the [CLS] attention takes no empty document");
            break;
        case FSGPU_LAB_BERT_LINEAR:
            if (N <= 0 || N > (1 << 20) || K <= 0 || K > (1 << 20)) return bad("bert stage: n and k must be in 1..=2^20");
            if (form == 0 ? (K % 32 != 0 || N % 64 != 0 || a.epilogue > 1) : (!fsgpu::bert_gemm_w_supported(N, K) || a.epilogue > 2))
                return bad("bert stage: linear shape or epilogue not supported by this form");
            break;
        case FSGPU_LAB_BERT_LINEAR_LN:
            if (K <= 0 || K > (1 << 20) || K % 32 != 0) return bad("bert stage: k must be a multiple of 32");
            if ((form == 0 && !fsgpu::bert_gemm_ln_supported(H)) || (form == 1 && !fsgpu::bert_gemm_ln_w_supported(H, K)))
                return bad("bert stage: linear + LayerNorm shape not supported by this form");
            break;
        case FSGPU_LAB_BERT_POST_ATTN:
            if (I <= 0 || I > (1 << 20)) return bad("bert stage: inter must be in 1..=2^20");
            if (form == 2 ? !(fsgpu::bert_gemm_ln_w_supported(H, H) && fsgpu::bert_ffn_w_supported(H, I)) : !fsgpu::bert_post_attn_w_supported(H, I))
                return bad("bert stage: post-attention shape not supported by this form");
            break;
        case FSGPU_LAB_BERT_EMBED_LN:
            if (form > 1 || a.vocab == 0 || a.max_pos == 0 || !a.ids || !a.positions || (form == 1 && (!a.types || !fsgpu::bert_rerank_supported(H))))
                return bad("bert stage: embedding needs ids, positions (and types), vocab and max_pos");
            for (uint32_t t = 0; t < a.m; ++t)
                if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos ||
                    (form == 1 && (a.types[t] < 0 || a.types[t] > 1)))
                    return bad("bert stage: token id, position or type out of range");
            break;
        case FSGPU_LAB_BERT_CLS_HEAD:
            break;
        default:
            if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq)) return bad("bert stage: offsets must run from 0 to m");
            break;
    }
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        const size_t m = a.m, h = a.hidden;
        if (st == FSGPU_LAB_BERT_ATTENTION) {
            const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
            const int heads = H / 32;
            if (form == 1) {
                const float* qkv = s.f32(a.in[0], m * 3 * h);
                void* ctx = s.out(m, h, 2, a.out0);
                if (s.ok()) s.hip(fsgpu::launch_bert_attention(qkv, offs, ctx, (int)a.n_docs, heads, H, (int)max_seq, a.scale, nullptr));
            } else if (form == 0) {
                const void* qkv = s.f16(a.in[0], m * 3 * h);
                void* ctx = s.out(m, h, 2, a.out0);
                if (s.ok()) s.hip(fsgpu::launch_bert_attention_h(qkv, offs, ctx, (int)a.n_docs, heads, H, (int)max_seq, a.scale, nullptr));
            } else {
                const void* qkv = s.f16(a.in[0], m * 3 * h);
                const float* x = s.f32(a.in[1], m * h);
                void* ctx = s.out(a.n_docs, h, 2, a.out0);
                float* x_cls = static_cast<float*>(s.out(a.n_docs, h, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_cls_attention(qkv, offs, x, ctx, x_cls, (int)a.n_docs, heads, H, a.scale, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_LINEAR) {
            const void* act = s.f16(a.in[0], m * a.k);
            const void* w = form == 0 ? s.f16(a.in[1], (size_t)a.n * a.k) : s.packed(a.in[1], N, K);
            const float* bias = s.f32(a.in[2], a.n);
            const bool half_out = a.epilogue != 0;
            void* y = s.out(m, a.n, half_out ? 2 : 4, a.out0);
            float* y32 = half_out ? nullptr : static_cast<float*>(y);
            void* y16 = half_out ? y : nullptr;
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_gemm(act, w, bias, y32, y16, M, N, K, a.epilogue == 1, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_gemm_w(act, w, bias, y32, y16, M, N, K, (int)a.epilogue, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_gemm_w_fixed(act, w, bias, y32, y16, M, N, K, (int)a.epilogue, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_LINEAR_LN) {
            const void* act = s.f16(a.in[0], m * a.k);
            const void* w = form == 1 ? s.packed(a.in[1], H, K) : s.f16(a.in[1], h * a.k);
            const float* bias = s.f32(a.in[2], h);
            const float* lnw = s.f32(a.in[4], h);
            const float* lnb = s.f32(a.in[5], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0, a.in[3]));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_gemm_ln(act, w, bias, x, x_h, lnw, lnb, M, H, K, a.eps, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_gemm_ln_w(act, w, bias, x, x_h, lnw, lnb, M, H, K, a.eps, nullptr));
            } else {
                float* tmp = static_cast<float*>(s.alloc(m * h * 4));
                if (s.ok()) s.hip(fsgpu::launch_bert_gemm(act, w, bias, tmp, nullptr, M, H, K, false, nullptr));
                if (s.ok()) s.hip(fsgpu::launch_bert_add_ln(x, tmp, lnw, lnb, x_h, M, H, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_POST_ATTN) {
            const size_t in = a.inter;
            const void* ctx = s.f16(a.in[0], m * h);
            const void* w0 = s.packed(a.in[1], H, H);
            const float* b0 = s.f32(a.in[2], h);
            const float* ln0w = s.f32(a.in[3], h);
            const float* ln0b = s.f32(a.in[4], h);
            const void* w1 = s.packed(a.in[5], I, H);
            const float* b1 = s.f32(a.in[6], in);
            const void* w2 = s.packed(a.in[7], H, I);
            const float* b2 = s.f32(a.in[8], h);
            const float* lnw = s.f32(a.in[9], h);
            const float* lnb = s.f32(a.in[10], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0, a.in[11]));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_post_attn_w(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_post_attn_w_fixed(ctx, w0, b0, ln0w, ln0b, w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_gemm_ln_w(ctx, w0, b0, x, x_h, ln0w, ln0b, M, H, H, a.eps, nullptr));
                if (s.ok()) s.hip(fsgpu::launch_bert_ffn_w(w1, b1, w2, b2, x, x_h, lnw, lnb, M, H, I, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_EMBED_LN) {
            const int32_t* ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
            const int32_t* positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
            const int32_t* types = form == 1 ? static_cast<const int32_t*>(s.raw(a.types, m * 4)) : nullptr;
            const float* word = s.f32(a.in[0], (size_t)a.vocab * h);
            const float* pos = s.f32(a.in[1], (size_t)a.max_pos * h);
            const float* type = s.f32(a.in[2], (form == 1 ? 2 : 1) * h);
            const float* lnw = s.f32(a.in[3], h);
            const float* lnb = s.f32(a.in[4], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out0));
            void* x_h = s.out(m, h, 2, a.out1);
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 0) {
                s.hip(fsgpu::launch_bert_embed_ln(ids, positions, word, pos, type, lnw, lnb, x, x_h, M, H, a.eps, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_embed_typed_ln(ids, types, positions, word, pos, type, lnw, lnb, x, x_h, M, H, a.eps, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_CLS_HEAD) {
            const float* x_cls = s.f32(a.in[0], m * h);
            const float* pool_w = s.f32(a.in[1], h * h);
            const float* pool_b = s.f32(a.in[2], h);
            const float* cls_w = s.f32(a.in[3], h);
            const float* cls_b = s.f32(a.in[4], 1);
            float* logits = static_cast<float*>(s.out(m, 1, 4, a.out0));
            float* scores = static_cast<float*>(s.out(m, 1, 4, a.out1));
            if (s.ok()) s.hip(fsgpu::launch_bert_cls_head(x_cls, pool_w, pool_b, cls_w, cls_b, logits, scores, M, H, nullptr));
        } else {
            const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
            const float* x = s.f32(a.in[0], m * h);
            float* pooled = static_cast<float*>(s.out(a.n_docs, h, 4, a.out0));
            if (s.ok()) s.hip(fsgpu::launch_bert_pool(x, offs, pooled, (int)a.n_docs, H, nullptr));
        }
        return s.status("bert stage: a kernel wrote into a guard band of its output");
    });
}

fsgpu_status fsgpu_lab_bert_int8_stage(int32_t device, const fsgpu_lab_bert_int8_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_int8_stage_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    const int M = (int)a.m, N = (int)a.n, K = (int)a.k, H = (int)a.hidden;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (st > FSGPU_LAB_BERT_I8_ADD_LN_QUANT) return bad("bert int8 stage: unknown stage");
    const bool two_forms = st == FSGPU_LAB_BERT_I8_QUANT_ROWS || st == FSGPU_LAB_BERT_I8_ADD_LN_QUANT;
    if (form > (two_forms ? 1u : 0u)) return bad("bert int8 stage: unknown form");
    static const int n_in[] = {1, 1, 3, 5, 4};
    for (int i = 0; i < n_in[st]; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert int8 stage: missing input");
    const bool no_q = st == FSGPU_LAB_BERT_I8_ADD_LN_QUANT && form == 1;
    const bool f32_out = st >= FSGPU_LAB_BERT_I8_GEMM, q_out = st != FSGPU_LAB_BERT_I8_GEMM && !no_q;
    if ((f32_out && !a.out_f32) || (q_out && (!a.out_codes || !a.out_scales)) || (st == FSGPU_LAB_BERT_I8_GEMM && !a.codes))
        return fail(FSGPU_ERR_NULL_ARGUMENT, "bert int8 stage: missing output or codes");
    if (st != FSGPU_LAB_BERT_I8_PACK_W && (a.m == 0 || a.m > (1u << 20))) return bad("bert int8 stage: m must be in 1..=2^20");
    if (st <= FSGPU_LAB_BERT_I8_GEMM) {
        // 127 x 127 x K < 2^31 (the i32 accumulator): K <= 4096 here
        if (K <= 0 || K % 64 != 0 || K > 4096) return bad("bert int8 stage: k must be a multiple of 64 and <= 4096");
        if (st != FSGPU_LAB_BERT_I8_QUANT_ROWS && (a.n > (1u << 20) || !fsgpu::bert_i8_gemm_supported(N, K)))
            return bad("bert int8 stage: n must be a multiple of 64");
        if (st == FSGPU_LAB_BERT_I8_GEMM && a.epilogue > 1) return bad("bert int8 stage: unknown epilogue");
    } else {
        if (H <= 0 || H % 64 != 0 || H > 1024) return bad("bert int8 stage: hidden must be a multiple of 64 and <= 1024");
        if (st == FSGPU_LAB_BERT_I8_EMBED_LN_QUANT) {
            if (a.vocab == 0 || a.max_pos == 0 || !a.ids || !a.positions) return bad("bert int8 stage: embedding needs ids, positions, vocab and max_pos");
            for (uint32_t t = 0; t < a.m; ++t)
                if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos)
                    return bad("bert int8 stage: token id or position out of range");
        }
    }
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        const size_t m = a.m, n = a.n, k = a.k, h = a.hidden;
        if (st == FSGPU_LAB_BERT_I8_QUANT_ROWS) {
            const void* x = form == 1 ? s.f16(a.in[0], m * k) : static_cast<const void*>(s.f32(a.in[0], m * k));
            void* q = s.out(m, k, 1, a.out_codes);
            float* sc = static_cast<float*>(s.out(m, 1, 4, a.out_scales));
            if (!s.ok()) {
                // (an upload failed: nothing is launched)
            } else if (form == 1) {
                s.hip(fsgpu::launch_bert_i8_quant_rows_h(x, q, sc, M, K, nullptr));
            } else {
                s.hip(fsgpu::launch_bert_i8_quant_rows(static_cast<const float*>(x), q, sc, M, K, nullptr));
            }
        } else if (st == FSGPU_LAB_BERT_I8_PACK_W) {
            const float* w = s.f32(a.in[0], n * k);
            void* wp = s.out(n, k, 1, a.out_codes);
            float* sw = static_cast<float*>(s.out(n, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_pack_w(w, wp, sw, N, K, nullptr));
        } else if (st == FSGPU_LAB_BERT_I8_GEMM) {
            const void* qa = s.raw(a.codes, m * k);
            const float* sa = s.f32(a.in[0], m);
            const float* w = s.f32(a.in[1], n * k);
            const float* bias = s.f32(a.in[2], n);
            void* wp = s.alloc(fsgpu::bert_i8_packed_bytes(N, K));
            float* sw = static_cast<float*>(s.alloc(n * 4));
            float* y = static_cast<float*>(s.out(m, n, 4, a.out_f32));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_pack_w(w, wp, sw, N, K, nullptr));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_gemm(qa, sa, wp, sw, bias, y, M, N, K, a.epilogue == 1, nullptr));
        } else if (st == FSGPU_LAB_BERT_I8_EMBED_LN_QUANT) {
            const int32_t* ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
            const int32_t* positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
            const float* word = s.f32(a.in[0], (size_t)a.vocab * h);
            const float* pos = s.f32(a.in[1], (size_t)a.max_pos * h);
            const float* type0 = s.f32(a.in[2], h);
            const float* lnw = s.f32(a.in[3], h);
            const float* lnb = s.f32(a.in[4], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out_f32));
            void* q = s.out(m, h, 1, a.out_codes);
            float* sc = static_cast<float*>(s.out(m, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_embed_ln_quant(ids, positions, word, pos, type0, lnw, lnb, x, q, sc, M, H, a.eps, nullptr));
        } else {
            const float* delta = s.f32(a.in[1], m * h);
            const float* lnw = s.f32(a.in[2], h);
            const float* lnb = s.f32(a.in[3], h);
            float* x = static_cast<float*>(s.out(m, h, 4, a.out_f32, a.in[0]));
            void* q = no_q ? s.out_untouched(m, h, 1) : s.out(m, h, 1, a.out_codes);
            float* sc = static_cast<float*>(no_q ? s.out_untouched(m, 1, 4) : s.out(m, 1, 4, a.out_scales));
            if (s.ok()) s.hip(fsgpu::launch_bert_i8_add_ln_quant(x, delta, lnw, lnb, no_q ? nullptr : q, sc, M, H, a.eps, nullptr));
        }
        return s.status("bert int8 stage: a kernel wrote into a guard band or into a buffer it must leave alone");
    });
}

fsgpu_status fsgpu_lab_bert_short_stage(int32_t device, const fsgpu_lab_bert_short_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_bert_short_args& a = *args;
    const uint32_t st = a.stage, form = a.form;
    auto bad = [](const char* what) { return fail(FSGPU_ERR_INVALID_CONFIG, what); };
    if (st > FSGPU_LAB_BERT_DOCS) return bad("bert short stage: unknown stage");
    const bool docs = st == FSGPU_LAB_BERT_DOCS;
    if (form > (st == FSGPU_LAB_BERT_Q_ATTN ? 1u : st == FSGPU_LAB_BERT_Q_GEMM ? 2u : 0u)) return bad("bert short stage: unknown form");
    if (!(docs ? fsgpu::bert_docs_w_supported((int)a.hidden, (int)a.inter, (int)a.heads)
               : fsgpu::bert_query_path_supported((int)a.hidden, (int)a.inter, (int)a.heads)))
        return bad("bert short stage: the short-text kernels are built for hidden 384, inter 1536, 12 heads");
    const bool embeds = docs || (st == FSGPU_LAB_BERT_Q_ATTN && form == 0);
    static const int n_in[4][3] = {{7, 7, 0}, {2, 7, 2}, {5, 0, 0}, {5, 0, 0}};
    for (int i = 0; i < n_in[st][form]; ++i)
        if (!a.in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: missing input");
    if (!a.out0) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: out0 is null");
    const bool two_outs = st == FSGPU_LAB_BERT_Q_ATTN || (st == FSGPU_LAB_BERT_Q_GEMM && form == 1);
    if (two_outs && !a.out1) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: out1 is null");
    if (a.m == 0 || a.m > (docs ? (1u << 20) : 32u)) return bad("bert short stage: m must be in 1..=32 (DOCS: 1..=2^20)");
    uint32_t max_seq = 0, min_seq = 0;
    if (!lab_offsets(a.offsets, a.n_docs, a.m, &max_seq, &min_seq)) return bad("bert short stage: offsets must run from 0 to m");
    if (docs && (max_seq > 32 || a.layers == 0 || a.layers > 6)) return bad("bert short stage: DOCS takes texts of at most 32 tokens and 1..=6 layers");
    if (docs) {
        if (!a.layer_in) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: layer_in is null");
        for (uint32_t i = 0; i < a.layers * 12; ++i)
            if (!a.layer_in[i]) return fail(FSGPU_ERR_NULL_ARGUMENT, "bert short stage: missing layer tensor");
    }
    if (embeds) {
        if (!a.ids || (!docs && !a.positions) || a.vocab == 0 || a.max_pos == 0 || a.max_pos > 512)
            return bad("bert short stage: embedding needs ids (, positions), vocab and max_pos in 1..=512");
        for (uint32_t t = 0; t < a.m; ++t)
            if (a.ids[t] < 0 || (uint32_t)a.ids[t] >= a.vocab || (!docs && (a.positions[t] < 0 || (uint32_t)a.positions[t] >= a.max_pos)))
                return bad("bert short stage: token id or position out of range");
        if (docs && max_seq > a.max_pos) return bad("bert short stage: text longer than max_pos");
    }
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        const size_t m = a.m, H = a.hidden, I = a.inter;
        const uint32_t* offs = static_cast<const uint32_t*>(s.raw(a.offsets, ((size_t)a.n_docs + 1) * 4));
        if (!docs) {
            // the argument block as NativeEmbedder::forward_query fills it
            fsgpu::BertQueryArgs q{};
            q.tokens = (int)a.m;
            q.n_docs = (int)a.n_docs;
            q.offsets = offs;
            q.eps = a.eps;
            q.attn_scale = a.scale;
            // the pending add + LayerNorm of `slabs` partial slabs: in[0..4]
            auto pending = [&](int slabs) {
                q.x_in = static_cast<const float*>(s.workspace(a.in[0], 1, m, H, false));
                q.parts = static_cast<const float*>(s.workspace(a.in[1], (size_t)slabs, m, H, false));
                q.n_parts = slabs;
                q.prev_bias = s.f32(a.in[2], H);
                q.lnw = s.f32(a.in[3], H);
                q.lnb = s.f32(a.in[4], H);
            };
            if (st == FSGPU_LAB_BERT_Q_ATTN) {
                if (form == 0) {
                    q.ids = static_cast<const int32_t*>(s.raw(a.ids, m * 4));
                    q.positions = static_cast<const int32_t*>(s.raw(a.positions, m * 4));
                    q.word = s.f32(a.in[0], (size_t)a.vocab * H);
                    q.pos = s.f32(a.in[1], (size_t)a.max_pos * H);
                    q.type0 = s.f32(a.in[2], H);
                    q.lnw = s.f32(a.in[3], H);
                    q.lnb = s.f32(a.in[4], H);
                } else {
                    pending(4);
                }
                q.w = static_cast<const _Float16*>(s.f16(a.in[5], 3 * H * H));
                q.ldw = (int)H;
                q.bias = s.f32(a.in[6], 3 * H);
                q.out_h = static_cast<_Float16*>(s.out(m, H, 2, a.out0));
                q.x_out = static_cast<float*>(s.out(m, H, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_qkv_attn(q, (int)a.heads, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM && form == 0) {
                q.a_h = static_cast<const _Float16*>(s.workspace(a.in[0], 1, m, H, true));
                q.lda = (int)H;
                q.w = static_cast<const _Float16*>(s.f16(a.in[1], H * H));
                q.ldw = (int)H;
                q.n = (int)H;
                q.out_f32 = static_cast<float*>(s.out(m, H, 4, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 0, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM && form == 1) {
                pending(1);
                q.w = static_cast<const _Float16*>(s.f16(a.in[5], I * H));
                q.ldw = (int)H;
                q.n = (int)I;
                q.bias = s.f32(a.in[6], I);
                q.out_h = static_cast<_Float16*>(s.out(m, I, 2, a.out0));
                q.x_out = static_cast<float*>(s.out(m, H, 4, a.out1));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 1, nullptr));
            } else if (st == FSGPU_LAB_BERT_Q_GEMM) {
                q.a_h = static_cast<const _Float16*>(s.workspace(a.in[0], 1, m, I, true));
                q.lda = (int)I;
                q.w = static_cast<const _Float16*>(s.f16(a.in[1], H * I));
                q.ldw = (int)I;
                q.n = (int)H;
                q.out_f32 = static_cast<float*>(s.out_slabs(4, m, H, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_gemm(q, 2, nullptr));
            } else {
                pending(4);
                float* pooled = static_cast<float*>(s.out(a.n_docs, H, 4, a.out0));
                if (s.ok()) s.hip(fsgpu::launch_bert_q_pool(q, pooled, nullptr));
            }
        } else {
            // the argument block as NativeEmbedder::embed_docs fills it, over the embedder's own row blocks
            const fsgpu::BertDocsPacking pk = fsgpu::bert_docs_pack(a.ids, a.offsets, a.n_docs, a.m);
            std::vector<unsigned char> host(pk.in_bytes);
            pk.fill(host.data(), a.offsets);
            fsgpu::BertDocsArgs d{};
            pk.point(d, static_cast<const unsigned char*>(s.raw(host.data(), host.size())));
            d.word = s.f32(a.in[0], (size_t)a.vocab * H);
            d.pos = s.f32(a.in[1], (size_t)a.max_pos * H);
            d.type0 = s.f32(a.in[2], H);
            d.emb_lnw = s.f32(a.in[3], H);
            d.emb_lnb = s.f32(a.in[4], H);
            std::vector<fsgpu::BertDocsLayer> table(a.layers);
            for (uint32_t l = 0; l < a.layers; ++l) {
                const float* const* t = a.layer_in + (size_t)l * 12;
                fsgpu::BertDocsLayer& L = table[l];
                L.qkv_wp = s.packed(t[0], 3 * (int)H, (int)H);
                L.qkv_b = s.f32(t[1], 3 * H);
                L.ao_wp = s.packed(t[2], (int)H, (int)H);
                L.ao_b = s.f32(t[3], H);
                L.ln1_w = s.f32(t[4], H);
                L.ln1_b = s.f32(t[5], H);
                L.i_wp = s.packed(t[6], (int)I, (int)H);
                L.i_b = s.f32(t[7], I);
                L.o_wp = s.packed(t[8], (int)H, (int)I);
                L.o_b = s.f32(t[9], H);
                L.ln2_w = s.f32(t[10], H);
                L.ln2_b = s.f32(t[11], H);
            }
            d.layers = static_cast<const fsgpu::BertDocsLayer*>(s.raw(table.data(), table.size() * sizeof(fsgpu::BertDocsLayer)));
            d.nlayers = (int)a.layers;
            d.eps = a.eps;
            d.attn_scale = a.scale;
            d.out = static_cast<float*>(s.out(a.n_docs, H, 4, a.out0));
            if (s.ok()) s.hip(fsgpu::launch_bert_docs_w(d, pk.nblocks, nullptr));
        }
        return s.status("bert short stage: a kernel wrote into a guard band of its output");
    });
}

fsgpu_status fsgpu_lab_scan_stage_check(const fsgpu_lab_scan_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return scan_stage_check(*args, nullptr);
}

int32_t fsgpu_lab_scan_planner_shape(int32_t requested, int32_t elem_bytes) { return fsgpu::scan_mfma_planner_shape(requested, elem_bytes); }

fsgpu_status fsgpu_lab_scan_stage(int32_t device, const fsgpu_lab_scan_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_scan_stage_args& a = *args;
    ScanStageGeom g;
    if (const fsgpu_status st = scan_stage_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        if (a.kernel == FSGPU_LAB_SCAN_PREPARE) {
            const size_t qn = (size_t)a.nq * a.dim;
            const float* q = a.nq ? s.f32(a.queries_f32, qn) : static_cast<const float*>(s.alloc(16));
            void* prepared = s.out_bytes((size_t)a.nq_pad * a.dim * a.elem_bytes, 0xCD, a.prepared);
            float* delta = static_cast<float*>(s.out_bytes((size_t)a.nq_pad * 4, 0xCD, a.delta));
            if (a.elem_bytes == 2) {
                const unsigned int* mx = static_cast<const unsigned int*>(s.raw(&a.max_norm_bits, 4));
                if (s.ok()) s.hip(fsgpu::launch_prepare_queries(q, a.nq, a.nq_pad, a.dim, 0, mx, prepared, delta, nullptr));
            } else if (s.ok()) {
                s.hip(fsgpu::launch_prepare_queries_i8(q, a.nq, a.nq_pad, a.dim, prepared, delta, nullptr, (int)a.bits));
            }
        } else {
            // the slab, with guard rows behind its last row: NaN halves / 0x7f bytes
            constexpr size_t kSlabGuardRows = 256;
            const size_t words = lab::bitmap_words(a.nrows);
            fsgpu::MfmaScanArgs m{};
            m.slab = s.with_tail(a.slab, (size_t)a.nrows * g.pitch, kSlabGuardRows * g.pitch, a.elem_bytes == 2 ? lab::Tail::kF16NaN : lab::Tail::kByte7f);
            m.live = s.bitmap(a.live, words);
            m.allow = s.bitmap(a.allow, words);
            m.queries = s.raw(a.queries, (size_t)a.nq_pad * a.dim * a.elem_bytes);
            if (a.tau) m.tau = static_cast<const float*>(s.raw(a.tau, (size_t)a.nq_pad * 4));
            m.cand = static_cast<fsgpu::u64*>(s.out_bytes(g.cand_n * 8, 0xCD, a.cand));
            m.cand_count = static_cast<uint32_t*>(s.out_bytes(g.count_n * 4, 0xCD, a.cand_count));
            m.dense = static_cast<fsgpu::u64*>(s.out_bytes(g.dense_n * 8, 0xCD, a.dense));
            if (g.lists) {
                m.spill = static_cast<fsgpu::u64*>(s.out_bytes(g.spill_n * 8, 0xCD, a.spill));
                m.spill_count = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq_pad * fsgpu::kMfmaSpillCountStride * 4, 0, a.spill_count));
                m.overflow = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq_pad * 4, 0, a.overflow));
            }
            m.spill_cap = a.spill_cap;
            m.nrows = a.nrows;
            m.stage = a.stage;
            m.group_stride = a.group_stride;
            m.group_count = a.group_count;
            m.dim = a.dim;
            m.slots = a.kernel == FSGPU_LAB_SCAN_REG && a.stage == 3 ? 4 : a.slots;
            m.row_base = a.row_base;
            m.elem_bytes = a.elem_bytes;
            m.reverse = a.reverse;
            m.row_stride = a.row_stride;
            m.groups = a.groups;
            m.side_by_side = a.side_by_side;
            if (s.ok()) {
                if (a.kernel == FSGPU_LAB_SCAN_LDS) s.hip(fsgpu::launch_scan_mfma(m, (int)a.variant, (int)a.grid, nullptr, nullptr));
                else s.hip(fsgpu::launch_scan_wide(m, (int)a.variant, (int)a.grid, nullptr, nullptr));
            }
        }
        return s.status("scan stage: a kernel wrote into a guard band of its output", "scan stage: the launcher refused the shape");
    });
}

fsgpu_status fsgpu_lab_select_check(const fsgpu_lab_select_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return select_check(*args, nullptr);
}

fsgpu_status fsgpu_lab_select(int32_t device, const fsgpu_lab_select_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_select_args& a = *args;
    SelectGeom g;
    if (const fsgpu_status st = select_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        auto in_u64 = [&](const uint64_t* src, size_t n) -> const fsgpu::u64* {
            return src && n ? static_cast<const fsgpu::u64*>(s.raw(src, n * 8)) : static_cast<const fsgpu::u64*>(s.alloc(16));
        };
        auto in_f32 = [&](const float* src, size_t n) -> const float* { return src && n ? s.f32(src, n) : nullptr; };
        // the slab with NaN guard rows behind its last row, the queries with NaN rows behind the last valid one
        constexpr size_t kGuardRows = 64;
        const void* slab = nullptr;
        const float* queries = nullptr;
        const fsgpu::u64 *live = nullptr, *allow = nullptr;
        if (g.finish) {
            slab = s.with_tail(a.slab, (size_t)a.nrows * g.slab_pitch, kGuardRows * g.slab_pitch, a.slab_f32 ? lab::Tail::kF32NaN : lab::Tail::kF16NaN);
            queries = static_cast<const float*>(s.with_tail(a.queries, g.query_rows * g.query_pitch * 4, kGuardRows * g.query_pitch * 4, lab::Tail::kF32NaN));
            live = s.bitmap(a.live, g.bitmap_words);
            allow = s.bitmap(a.allow, g.bitmap_words);
        }
        const fsgpu::u64* lists = in_u64(a.lists, g.lists_n);
        uint32_t* spill_count = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * fsgpu::kMfmaSpillCountStride * 4, 0, a.spill_count, true));
        float* tau_out = static_cast<float*>(s.out_bytes((a.kernel == FSGPU_LAB_LIST_CUT ? 1 : (size_t)a.nq) * 4, 0xCD, a.tau_out));
        uint32_t* overflow = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0, a.overflow));
        if (a.kernel == FSGPU_LAB_SELECT) {
            fsgpu::SelectArgs m{};
            m.lists = lists;
            m.q_stride = a.q_stride;
            m.l_stride = a.l_stride, m.nlists = a.nlists, m.list_len = a.list_len;
            m.list_counts = a.list_counts && g.counts_n ? static_cast<const uint32_t*>(s.raw(a.list_counts, g.counts_n * 4)) : nullptr;
            m.extra = a.extra_len ? in_u64(a.extra, (size_t)a.nq * a.extra_len) : nullptr;
            m.extra_len = a.extra_len;
            m.spill = a.spill ? in_u64(a.spill, (size_t)a.nq * a.spill_cap) : nullptr;
            m.spill_count = spill_count;
            m.spill_cap = a.spill_cap;
            m.k = a.k;
            m.spill_reset = a.reset_spill ? spill_count : nullptr;
            m.delta = in_f32(a.delta, a.nq);
            m.tau_out = tau_out;
            m.pool_out = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * fsgpu::kSelectPool * 8, 0xCD, a.pool_out));
            m.cand_counts = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0xCD, a.cand_counts));
            m.overflow = overflow;
            m.take_topk = a.take_topk;
            m.anchor_unit = in_f32(a.anchor_unit, a.nq);
            m.heur_rank = a.heur_rank;
            m.tau_floor_out = static_cast<float*>(s.out_bytes((size_t)a.nq * 4, 0xCD, a.tau_floor_out));
            m.tau_floor_in = in_f32(a.tau_floor_in, a.nq);
            m.pool_flag = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0, a.pool_flag, true));
            m.slab = slab;
            m.queries = queries;
            m.dim = a.dim, m.nrows = a.nrows, m.row_base = a.row_base, m.row_stride = a.row_stride, m.query_stride = a.query_stride;
            m.hreduce = a.hreduce;
            m.k_out = a.k_out, m.out_stride = a.out_stride;
            m.out_rows = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_rows));
            m.out_scores = static_cast<float*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_scores));
            m.out_packed = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * a.out_stride * 8, 0xCD, a.out_packed));
            m.out_counts = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0xCD, a.out_counts));
            m.cand_approx_out = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * a.cand_out_stride * 8, 0xCD, a.cand_approx_out));
            m.cand_exact_out = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * a.cand_out_stride * 8, 0xCD, a.cand_exact_out));
            m.cand_out_stride = a.cand_out_stride;
            m.valid_queries = a.valid_queries;
            m.slab_f32 = a.slab_f32;
            if (s.ok() && a.big_pool != 2) s.hip(fsgpu::launch_select(m, (int)a.nq, nullptr));
            if (s.ok() && a.big_pool != 0) {
                m.big_pool = 1;
                s.hip(fsgpu::launch_select(m, (int)a.nq, nullptr));
            }
        } else if (a.kernel == FSGPU_LAB_SELECT_GROUPS) {
            fsgpu::GroupSelectArgs m{};
            m.groups = lists;
            m.nentries = a.nentries;
            m.k = a.k;
            m.delta = in_f32(a.delta, a.nq);
            m.anchor_unit = in_f32(a.anchor_unit, a.nq);
            m.tau_out = tau_out;
            m.overflow = overflow;
            m.spill_reset = a.reset_spill ? spill_count : nullptr;
            m.slab = slab;
            m.live = live, m.allow = allow;
            m.queries = queries;
            m.dim = a.dim, m.nrows = a.nrows, m.row_base = a.row_base, m.query_stride = a.query_stride;
            m.hreduce = a.hreduce;
            m.valid_queries = a.valid_queries;
            m.slab_f32 = a.slab_f32;
            m.rank_only = a.rank_only;
            if (s.ok()) s.hip(fsgpu::launch_select_groups(m, (int)a.nq, nullptr));
        } else if (a.kernel == FSGPU_LAB_LIST_CUT) {
            if (s.ok()) s.hip(fsgpu::launch_list_cut(lists, a.nlists, a.list_len, tau_out, nullptr));
        } else {
            const fsgpu::u64* exact = in_u64(a.exact_lists, g.exact_n);
            uint32_t* rows = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_rows));
            float* scores = static_cast<float*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_scores));
            uint32_t* counts = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0xCD, a.out_counts));
            if (s.ok()) s.hip(fsgpu::launch_two_pass_merge(lists, exact, a.nshards, a.shard_pitch, a.nq, a.cc, a.k, a.out_stride, rows, scores, counts, nullptr));
        }
        return s.status("select: a kernel wrote into a guard band of its output", "select: the launcher refused the arguments");
    });
}

fsgpu_status fsgpu_lab_lone_stage_check(const fsgpu_lab_lone_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return lone_stage_check(*args, nullptr);
}

fsgpu_status fsgpu_lab_lone_stage(int32_t device, const fsgpu_lab_lone_stage_args* args) {
    if (!args) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    const fsgpu_lab_lone_stage_args& a = *args;
    LoneGeom g;
    if (const fsgpu_status st = lone_stage_check(a, &g); st != FSGPU_OK) return st;
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        if (a.kind == FSGPU_LAB_LONE_MERGE) {
            fsgpu::MergeArgs m;
            m.lists = static_cast<const fsgpu::u64*>(s.raw(a.lists, g.lists_n * 8));
            m.q_stride = a.q_stride;
            m.l_stride = a.l_stride;
            m.nlists = a.nlists;
            m.list_len = a.list_len;
            m.k = a.k;
            m.out_stride = a.out_stride;
            m.out_rows = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_rows));
            m.out_scores = static_cast<float*>(s.out_bytes((size_t)a.nq * a.out_stride * 4, 0xCD, a.out_scores));
            m.out_counts = static_cast<uint32_t*>(s.out_bytes((size_t)a.nq * 4, 0xCD, a.out_counts));
            m.out_packed = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * a.out_stride * 8, 0xCD, a.out_packed));
            m.lists_sorted = a.lists_sorted;
            if (s.ok()) s.hip(fsgpu::launch_merge_topk(m, (int)a.nq, nullptr));
        } else {
            // the slab with guard rows behind its last row: NaN (f16 0x7e00, f32 0x7fc00000) or 0x7f (int8, 4-bit)
            constexpr size_t kGuardRows = 64;
            const lab::Tail tail = a.kind == FSGPU_LAB_LONE_F32 ? lab::Tail::kF32NaN : a.kind <= FSGPU_LAB_LONE_F16_MQ ? lab::Tail::kF16NaN : lab::Tail::kByte7f;
            const void* slab = s.with_tail(a.slab, (size_t)a.nrows * g.slab_pitch, kGuardRows * g.slab_pitch, tail);
            const bool host_query = a.kind == FSGPU_LAB_LONE_F16_HOST_QUERY;
            const void* query = host_query ? nullptr : s.raw(a.queries, g.query_bytes);
            const bool quantised = a.kind == FSGPU_LAB_LONE_I8 || a.kind == FSGPU_LAB_LONE_I4;
            fsgpu::ScanArgs m{};
            m.slab = quantised ? nullptr : slab;
            m.live = s.bitmap(a.live, g.bitmap_words);
            m.allow = s.bitmap(a.allow, g.bitmap_words);
            m.queries = quantised || host_query ? nullptr : static_cast<const float*>(query);
            m.partial = static_cast<fsgpu::u64*>(s.out_bytes((size_t)a.nq * a.grid * a.k * 8, 0xCD, a.partial));
            m.nrows = a.nrows;
            m.dim = a.dim;
            m.k = a.k;
            m.row_base = a.row_base;
            m.hreduce = a.hreduce;
            m.row_stride = (uint32_t)g.slab_pitch;
            const int nq = (int)a.nq, tier = (int)a.tier, grid = (int)a.grid;
            if (s.ok()) {
                switch (a.kind) {
                    case FSGPU_LAB_LONE_F16: s.hip(fsgpu::launch_scan_topk(m, nq, tier, grid, nullptr, a.force_runtime_dim != 0, a.plain_loads != 0)); break;
                    case FSGPU_LAB_LONE_F16_HOST_QUERY: s.hip(fsgpu::launch_scan_topk_host_query(m, static_cast<const float*>(a.queries), tier, grid, nullptr)); break;
                    case FSGPU_LAB_LONE_F16_MQ: s.hip(fsgpu::launch_scan_mq(m, nq, tier, grid, nullptr, nullptr)); break;
                    case FSGPU_LAB_LONE_I8: s.hip(fsgpu::launch_scan_i8(m, slab, query, tier, grid, nullptr, nullptr)); break;
                    case FSGPU_LAB_LONE_I4: s.hip(fsgpu::launch_scan_4bit(m, slab, query, tier, grid, nullptr, nullptr)); break;
                    default: s.hip(fsgpu::launch_scan_topk_f32(m, tier, nq, grid, nullptr, nullptr)); break;
                }
            }
        }
        return s.status("lone: a kernel wrote into a guard band of its output", "lone: the launcher refused the arguments");
    });
}

fsgpu_status fsgpu_lab_knn_update_join(int32_t device, const void* slab, uint32_t slab_f32, uint32_t nrows, uint32_t dim, int32_t hreduce,
                                       uint32_t m, const uint8_t* classes, uint64_t* work, const float* added, const uint32_t* added_rows,
                                       uint32_t n_added) {
    if (!slab || !classes || !work || !added || !added_rows) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (m < 1 || m > fsgpu::kKnnMaxM || dim < 1 || dim > fsgpu::kKnnUpdMaxDim || nrows < 1 || nrows > (1u << 24) || n_added < 1 ||
        n_added > fsgpu::kKnnUpdBlock || hreduce < 0 || hreduce > 2)
        return fail(FSGPU_ERR_INVALID_CONFIG, "knn update join: m 1..63, dim 1..1024, 1..2^24 rows, 1..1024 added rows, hreduce 0..2");
    return guarded([&]() -> fsgpu_status {
        if (const fsgpu_status opened = LabStage::open(device); opened != FSGPU_OK) return opened;
        LabStage s;
        const size_t pitch = (size_t)dim * (slab_f32 ? 4 : 2);
        fsgpu::KnnUpdJoinArgs a{};
        a.slab = s.with_tail(slab, (size_t)nrows * pitch, LabStage::kGuardRows * pitch, slab_f32 ? lab::Tail::kF32NaN : lab::Tail::kF16NaN);
        a.row_stride = (uint32_t)pitch;
        a.dim = dim;
        a.slab_f32 = slab_f32 ? 1u : 0u;
        a.hreduce = hreduce;
        a.row0 = 0;
        a.nrows = nrows;
        a.m = m;
        a.cls = static_cast<const uint8_t*>(s.raw(classes, nrows));
        a.work = static_cast<fsgpu::u64*>(s.out_bytes((size_t)nrows * m * 8, 0, work, true));
        a.added = s.f32(added, (size_t)n_added * dim);
        a.added_rows = static_cast<const uint32_t*>(s.raw(added_rows, (size_t)n_added * 4));
        a.n_added = n_added;
        if (s.ok()) s.hip(fsgpu::launch_knn_update_join(a, nullptr));
        return s.status("knn update join: the kernel wrote into a guard band of the working table", "knn update join: the launcher refused the shape");
    });
}

// ---- the IVF index's int8 list filter ----
fsgpu_status fsgpu_lab_ivf_filter_stage(fsgpu_ivf* ivf, const fsgpu_lab_ivf_filter_stage_args* a) {
    if (!ivf || !a || !a->queries || !a->out_delta || !a->out_ran || !a->out_nslots || !a->out_slot_query || !a->out_slot_list ||
        !a->out_slot_offset || !a->out_scores || !a->out_t || !a->out_m || !a->out_count || !a->out_flag || !a->out_cand)
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (a->nq < 1) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter stage: no query");
    return guarded([&]() -> fsgpu_status {
        std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
        std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
        if (const fsgpu_status opened = LabStage::open(ivf->impl.device()); opened != FSGPU_OK) return opened;
        LabStage s;
        std::vector<unsigned char> host[6];
        fsgpu::IvfFilterLab flab;
        flab.alloc = [&](fsgpu::IvfFilterLab::Which w, size_t bytes) -> void* {
            host[w].assign(bytes, 0);
            void* p = s.out_bytes(bytes, lab::kGuardByte, host[w].data());
            s.hip(hipDeviceSynchronize());   // (the prefill ran on the null stream, the search runs on the index's)
            return s.ok() ? p : nullptr;
        };
        const size_t hits = (size_t)a->nq * std::max<uint32_t>(a->k, 1);
        std::vector<uint32_t> rows(hits), counts(a->nq), flags(a->nq);
        std::vector<float> scores(hits);
        const fsgpu::SearchError e = ivf->impl.search(a->queries, a->nq, a->query_len, a->k, a->nprobe, rows.data(), scores.data(), counts.data(),
                                                     flags.data(), false, nullptr, &flab);
        if (!e.ok()) return finish(e);
        const fsgpu_status st = s.status("ivf filter: a kernel wrote into a guard band of its output");
        if (st != FSGPU_OK) return st;
        std::memcpy(a->out_delta, flab.delta.data(), (size_t)a->nq * 4);
        *a->out_ran = flab.ran ? 1u : 0u;
        *a->out_nslots = 0;
        if (a->out_ordered) {
            const fsgpu::SearchError eo = ivf->impl.filter_ordered_copy(reinterpret_cast<signed char*>(a->out_ordered));
            if (!eo.ok()) return finish(eo);
        }
        if (!flab.ran) return FSGPU_OK;
        const uint32_t slots = (uint32_t)flab.slot_query.size();
        if (slots > a->slots_cap) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter stage: slots_cap is below the call's slots");
        const int32_t* sc = reinterpret_cast<const int32_t*>(host[fsgpu::IvfFilterLab::kScores].data());
        uint64_t off = 0;
        for (uint32_t sl = 0; sl < slots; ++sl) {
            const fsgpu::IvfFilterTile& t = flab.tiles[flab.slot_tile[sl]];
            const uint64_t len_pad = fsgpu::ivf_filter::round_up(t.len, fsgpu::kIvfFilterRowTile);
            const int32_t* src = sc + t.scratch0 + (uint64_t)(sl - t.slot0) * len_pad;
            if (off + t.len > a->scores_cap) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter stage: scores_cap is below the call's scores");
            a->out_slot_offset[sl] = off;
            std::memcpy(a->out_scores + off, src, (size_t)t.len * 4);
            for (uint64_t i = t.len; i < len_pad; ++i)
                if (src[i] != fsgpu::kIvfFilterDead) return fail(FSGPU_ERR_DEVICE, "ivf filter: a padding row of the scores is not the sentinel");
            off += t.len;
        }
        a->out_slot_offset[slots] = off;
        std::memcpy(a->out_slot_query, flab.slot_query.data(), (size_t)slots * 4);
        std::memcpy(a->out_slot_list, flab.slot_list.data(), (size_t)slots * 4);
        std::memcpy(a->out_t, host[fsgpu::IvfFilterLab::kT].data(), (size_t)slots * 4);
        std::memcpy(a->out_m, host[fsgpu::IvfFilterLab::kM].data(), (size_t)slots * 8);
        std::memcpy(a->out_count, host[fsgpu::IvfFilterLab::kCount].data(), (size_t)slots * 4);
        std::memcpy(a->out_flag, host[fsgpu::IvfFilterLab::kFlag].data(), (size_t)slots * 4);
        std::memcpy(a->out_cand, host[fsgpu::IvfFilterLab::kCand].data(), (size_t)slots * fsgpu::kIvfFilterSlotCap * 4);
        *a->out_nslots = slots;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_ivf_filter_set_scratch(fsgpu_ivf* ivf, uint64_t entries) {
    if (!ivf) return fail(FSGPU_ERR_NULL_ARGUMENT, "handle is null");
    std::shared_lock<std::shared_mutex> state(ivf->idx->state_mu);
    std::lock_guard<std::mutex> lock(ivf->idx->impl.mutex());
    ivf->impl.set_filter_scratch_entries(entries);
    return FSGPU_OK;
}

extern "C++" {
namespace {
fsgpu::ivf_filter::Caps lab_filter_caps(uint64_t scratch_cap) {
    return fsgpu::ivf_filter::Caps{scratch_cap ? scratch_cap : fsgpu::kIvfFilterScratchEntries, fsgpu::kIvfFilterTileQueries, fsgpu::kIvfFilterRowTile,
                                   fsgpu::kIvfFilterItemRows, fsgpu::kIvfFilterSlotCap};
}
std::vector<uint32_t> lab_filter_head(uint32_t nlist, const uint32_t* members) {
    std::vector<uint32_t> head((size_t)nlist + 1, 0u);
    for (uint32_t l = 0; l < nlist; ++l) head[l + 1] = head[l] + members[l];
    return head;
}
}  // namespace
}  // extern "C++"

fsgpu_status fsgpu_lab_ivf_filter_score_plan(uint32_t nlist, const uint64_t* offsets, const uint32_t* members, uint64_t scratch_cap, uint32_t tiles_cap,
                                             uint64_t* out_tiles, uint32_t* out_ntiles, uint32_t ranges_cap, uint64_t* out_ranges,
                                             uint32_t* out_nranges, uint32_t* out_slots) {
    if (!offsets || !members || !out_tiles || !out_ntiles || !out_ranges || !out_nranges || !out_slots)
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    return guarded([&]() -> fsgpu_status {
        uint64_t total = 0;
        const std::vector<uint64_t> first = fsgpu::ivf_filter::pad_rows(nlist, offsets, fsgpu::kIvfFilterRowTile, &total);
        const std::vector<uint32_t> head = lab_filter_head(nlist, members);
        const fsgpu::ivf_filter::ScorePlan p = fsgpu::ivf_filter::score_plan(nlist, offsets, head.data(), first.data(), lab_filter_caps(scratch_cap));
        const uint32_t ntiles = (uint32_t)p.tiles.size() - 1;
        if (ntiles > tiles_cap || p.ranges.size() > ranges_cap) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter plan: an output capacity is too small");
        for (uint32_t t = 0; t < ntiles; ++t) {
            const fsgpu::IvfFilterTile& x = p.tiles[t];
            const uint64_t row[8] = {x.ordered_row0, x.list_pos0, x.scratch0, x.len, x.slot0, x.nmem, x.item0, p.above[t]};
            std::memcpy(out_tiles + (size_t)t * 8, row, sizeof(row));
        }
        for (size_t r = 0; r < p.ranges.size(); ++r) {
            const fsgpu::ivf_filter::Range& x = p.ranges[r];
            const uint64_t row[7] = {x.tile_first, x.ntiles, x.item_first, x.nitems, x.slot_first, x.nslots, x.entries};
            std::memcpy(out_ranges + r * 7, row, sizeof(row));
        }
        *out_ntiles = ntiles;
        *out_nranges = (uint32_t)p.ranges.size();
        *out_slots = p.slots;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_ivf_filter_scan_plan(uint32_t nlist, const uint64_t* offsets, const uint32_t* members, const uint32_t* counts,
                                            const uint32_t* flags, uint32_t k, uint32_t num_cus, uint32_t groups_cap, uint64_t* out_groups,
                                            uint32_t* out_ngroups, uint32_t* out_grid_x, uint64_t* out_rows_rescored) {
    if (!offsets || !members || !counts || !flags || !out_groups || !out_ngroups || !out_grid_x || !out_rows_rescored)
        return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (k < 1) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter plan: k is 0");
    return guarded([&]() -> fsgpu_status {
        const std::vector<uint32_t> head = lab_filter_head(nlist, members);
        const fsgpu::ivf_filter::ScanPlan p =
            fsgpu::ivf_filter::scan_plan(nlist, offsets, head.data(), counts, flags, k, num_cus, fsgpu::kGatherTileRows, lab_filter_caps(0));
        if (p.groups.size() > groups_cap) return fail(FSGPU_ERR_INVALID_CONFIG, "ivf filter plan: an output capacity is too small");
        for (size_t g = 0; g < p.groups.size(); ++g) {
            const fsgpu::ivf_filter::Group& x = p.groups[g];
            const uint64_t row[6] = {x.rows_off, x.from_cand, x.n, x.q0, x.nq, x.nblocks};
            std::memcpy(out_groups + g * 6, row, sizeof(row));
        }
        *out_ngroups = (uint32_t)p.groups.size();
        *out_grid_x = p.grid_x;
        *out_rows_rescored = p.rows_rescored;
        return FSGPU_OK;
    });
}

fsgpu_status fsgpu_lab_hash_embed_stage_ms(fsgpu_hash* h, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n, float* out,
                                           float* out_stage_ms) {
    if (!h || !out_stage_ms) return fail(FSGPU_ERR_NULL_ARGUMENT, "null argument");
    if (n && !out) return fail(FSGPU_ERR_NULL_ARGUMENT, "out is null");
    return guarded([&]() -> fsgpu_status {
        return finish(h->impl.embed_batch(text_bytes, offsets, n, out, nullptr, nullptr, nullptr, out_stage_ms));
    });
}

fsgpu_status fsgpu_lab_wordpiece_encode_stage_ms(fsgpu_wordpiece* tok, const uint8_t* text_bytes, const uint32_t* offsets, uint32_t n,
                                                 int32_t add_special_tokens, uint32_t max_length, uint32_t* out_ids, uint64_t ids_capacity,
                                                 uint32_t* out_offsets, float* out_stage_ms) {
    if (!out_stage_ms) return fail(FSGPU_ERR_NULL_ARGUMENT, "out_stage_ms is null");
    fsgpu::WordPieceTokenizer::Request r;
    r.a_bytes = text_bytes;
    r.a_offsets = offsets;
    r.n = n;
    r.add_special = add_special_tokens != 0;
    r.max_length = max_length;
    r.ids_capacity = ids_capacity;
    r.out_ids = out_ids;
    r.out_offsets = out_offsets;
    r.stage_ms = out_stage_ms;
    return wordpiece_encode(tok, r);
}

}  // extern "C"

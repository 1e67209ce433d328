// kernels.hpp — argument blocks and host launchers of the fsgpu HIP kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "ivf_filter_tile.hpp"

namespace fsgpu {

typedef unsigned long long u64;

struct ScanArgs {
    const void* slab;       // [nrows, dim] little-endian f16, row-major (FSVI slab, lib.rs:36-41)
    const u64* live;        // bit r set = row r live (tombstone flag clear); nullptr = all live
    const u64* allow;       // per-call filter bitmap; nullptr = no filter
    const float* queries;   // [nq, dim] f32 (device)
    u64* partial;           // [nq, grid, k] packed best-first lists (device)
    uint32_t nrows;
    uint32_t dim;
    uint32_t k;
    uint32_t row_base;      // added to local rows (shard offset)
    int32_t hreduce;        // FSGPU_HREDUCE_*
    uint32_t row_stride;    // bytes between rows (>= dim*2); the MRL truncated scan reads a prefix of every row
};

struct MergeArgs {
    const u64* lists;       // packed entries; element (q, l, i) at lists[q*q_stride + l*l_stride + i]
    uint64_t q_stride;
    uint64_t l_stride;
    uint32_t nlists;
    uint32_t list_len;
    uint32_t k;             // entries to select per query
    uint32_t out_stride;    // row stride of the outputs (>= k); slots beyond the count are padded
    uint32_t* out_rows;     // [nq, out_stride]
    float* out_scores;      // [nq, out_stride]
    uint32_t* out_counts;   // [nq]
    u64* out_packed;        // optional [nq, out_stride] packed copy of the result (kEmpty padded)
    uint32_t lists_sorted = 1;  // 0: the lists are NOT best-first (disables the head/tail pruning bounds)
};

size_t scan_lds_bytes(int dim, int nq, int kcap);
int scan_occupancy_blocks_per_cu(int dim, int nq, int kcap, bool force_runtime_dim);
hipError_t launch_scan_topk(const ScanArgs& args, int nq, int kcap, int grid, hipStream_t stream,
                            bool force_runtime_dim, bool plain_loads);
// scan_mq_kernel.hip: 4 / 8 queries per pass (dim 128/256/384); occupancy != nullptr only queries residency.
bool scan_mq_supported(int dim, int nq, int kcap);
hipError_t launch_scan_mq(const ScanArgs& args, int nq, int kcap, int grid, hipStream_t stream, int* occupancy);
hipError_t launch_merge_topk(const MergeArgs& args, int nq, hipStream_t stream);
// one query read from HOST memory at launch time (it travels in the kernel's argument block: no H2D copy); dim <= 512, kcap 64 / 256
constexpr int kKernargQueryDims = 512;
bool scan_kernarg_query_supported(int dim, int kcap);
hipError_t launch_scan_topk_host_query(const ScanArgs& args, const float* query_host, int kcap, int grid, hipStream_t stream);
hipError_t launch_score_rows(const ScanArgs& args, u64* out_packed, int q_index, int grid, hipStream_t stream);
hipError_t launch_packed_to_sortkey(u64* data, size_t n, hipStream_t stream);
hipError_t launch_sorted_keys_to_rows(const u64* keys, uint32_t k, uint32_t* out_rows, uint32_t* out_count,
                                      hipStream_t stream, u64* out_packed = nullptr);
hipError_t launch_gather_dot(const ScanArgs& args, const uint32_t* rows, uint32_t n, float* out, hipStream_t stream);
// (rows[i], qidx[i]) items against args.queries = [nq, dim]: one launch for a chunk of queries (dim % 8 == 0, f16 rows)
hipError_t launch_gather_dot_mq(const ScanArgs& args, const uint32_t* rows, const uint32_t* qidx, uint32_t n, float* out, hipStream_t stream);
hipError_t launch_gather_queries(const float* src, const uint32_t* idx, uint32_t n, uint32_t dim, uint32_t src_stride, float* dst,
                                 hipStream_t stream);
hipError_t launch_scatter_hits(const uint32_t* idx, uint32_t n, uint32_t k, const uint32_t* src_rows,
                               const float* src_scores, const uint32_t* src_counts, uint32_t* dst_rows,
                               float* dst_scores, uint32_t* dst_counts, u64* dst_packed, hipStream_t stream);
hipError_t launch_encode_f16(const float* src, size_t n, unsigned short* dst, hipStream_t stream);
// The reference's bench corpus / queries (frankensearch/benches/fsvi_4bit_vs_incumbent.rs:56-101,344-365) written straight into
// device memory: vectors first .. first+n with seeds seed_base + index, as f16 rows (out_f16) or f32 queries (out_f32).
// centroid_scratch holds clusters * dim floats.
hipError_t launch_bench_fixture(uint64_t first, uint64_t n, uint32_t dim, uint32_t clusters, float noise, uint64_t seed_base,
                                float* centroid_scratch, unsigned short* out_f16, float* out_f32, hipStream_t stream);
hipError_t launch_encode_rows_f16(const float* src, const uint32_t* perm, uint64_t n, uint32_t dim, unsigned short* dst,
                                  hipStream_t stream);
hipError_t launch_widen_f16(const unsigned short* src, size_t n, float* dst, hipStream_t stream);

// f32_kernels.hip — Quantization::F32 slabs: every row's packed (score, row) entry, and the gathered dot
// fused scan + top-k over an F32 slab (one query per pass; lists to args.partial like launch_scan_topk); kcap 64 / 256
hipError_t launch_scan_topk_f32(const ScanArgs& args, int kcap, int nq, int grid, hipStream_t stream, int* occupancy);
int scan_f32_queries_per_pass(int dim, int kcap, int want);   // 4, 2 or 1: what the LDS holds
hipError_t launch_score_rows_f32(const ScanArgs& args, u64* out_packed, int q_index, hipStream_t stream);
hipError_t launch_gather_dot_f32(const ScanArgs& args, const uint32_t* rows, uint32_t n, float* out, hipStream_t stream);

// sort_general.hip (own LSD radix sort, descending u64 keys) — the large-k / collect-all path.
// varying_bits: the key bits that can differ between two keys of the input (digits without any are skipped).
hipError_t sort_keys_desc_temp_bytes(size_t n, size_t* temp_bytes);
hipError_t sort_keys_desc(void* temp, size_t temp_bytes, const u64* keys_in, u64* keys_out, size_t n,
                          hipStream_t stream, u64 varying_bits = ~0ull);

// m2v_kernels.hip
hipError_t launch_m2v_embed(const float* table, uint32_t vocab, uint32_t dim, const uint32_t* ids,
                            const uint32_t* offsets, uint32_t n, float* out, hipStream_t stream);

// mfma_scan.hip — batched approximate scan on the matrix cores + exact re-score helpers
struct MfmaScanArgs {
    const void* slab;          // [nrows, dim] f16
    const u64* live;           // may be null
    const u64* allow;          // may be null
    const void* queries;       // [nq_pad, dim] f16 (rows >= nq are zero)
    const float* tau;          // [nq_pad] candidate threshold per query (ignored in dense mode)
    u64* cand;                 // [nq_pad, gridDim.x, slots] packed approximate candidates, one list per block
    u64* spill;                // [nq_pad, spill_cap] candidates that did not fit their block's list
    uint32_t* spill_count;     // [nq_pad * kMfmaSpillCountStride] append counters, one cache line apart
    uint32_t spill_cap;
    uint32_t* overflow;        // [nq_pad] set when a query's spill area overflows too
    u64* dense;                // stage 0: [nq_pad, group_count * 64] packed approximate scores of the sample
    uint32_t nrows;            // rows in the slab
    uint32_t stage;            // 0 = dense sample, 1 = thresholded sample, 2 = main pass (everything stage 1 skipped),
                               // 3 = (mfma_wide.hip, int8 rows) sample that writes each block's four best GROUPS per query into cand
                               //     ([q][block][4]: best approximate score | first row of the group's 8 rows) — no thresholds, no lists
    uint32_t group_stride, group_count;  // the sample, in 64-row groups: {j * group_stride : j < group_count}
    uint32_t dim, slots, row_base;       // slots <= kMfmaMaxSlots
    uint32_t elem_bytes;                 // 2 = f16 slab / f16 queries (0 means 2), 1 = int8 slab / int8 queries
    uint32_t reverse;                    // main pass: walk the slab from its end (alternate passes re-read what the
                                         // previous pass left in the Infinity Cache)
    uint32_t row_stride;                 // bytes between rows; 0 = dense (dim * elem_bytes).  MRL prefix views scan the first
                                         // dim dimensions of rows that are row_stride bytes apart
    uint32_t groups;                     // sample stages: query groups answered by one launch (gridDim.y; 0 means 1) —
                                         // group g's queries/tau/cand/spill/overflow/dense follow group g-1's
    uint32_t* cand_count;                // mfma_wide.hip: [nq_pad, gridDim.x] entries in each (query, block) list, clamped to
                                         // slots (may be null: the lists are then padded with kEmpty instead)
    uint32_t side_by_side;               // mfma_wide.hip main pass, groups > 1: the groups run concurrently on gridDim.x walkers each and
                                         // walk the slab in the same direction (0: one after the other, alternating directions)
};

// select_kernel (mfma_scan.hip): per query, the k-th best of the packed approximate entries without sorting them
// (k rounds of wave arg-max per wave, k more over the 16 waves' winners) -> tau = a_k - 2 delta; the entries at or
// above tau are the query's candidates.  Two uses:
//   threshold step (slab == null): tau_out for the next scan stage, candidates optionally kept as a pool;
//   finish step (slab != null): the <= kSelectPool candidates are re-scored with the exact-order dot right in the block (one
//   quad per candidate) and the best k_out exact entries are emitted best first.
struct SelectArgs {
    const u64* lists;          // [nq][nlists][list_len] (strides below), kEmpty = hole
    uint64_t q_stride;         // entries between queries
    uint32_t l_stride, nlists, list_len;
    const uint32_t* list_counts;  // [nq][nlists] valid entries at the head of each list (may be null: every slot is read and
                                  // kEmpty marks the holes) — the register-resident-query scan writes counts instead of padding
    const u64* extra;          // [nq, extra_len] more entries per query (may be null)
    uint32_t extra_len;
    const u64* spill;          // [nq, spill_cap] spilled entries (may be null); valid prefix = min(count, spill_cap)
    const uint32_t* spill_count;  // [nq * kMfmaSpillCountStride]
    uint32_t spill_cap;
    uint32_t k;                // 1..kSelectMaxK
    uint32_t* spill_reset;     // [nq * kMfmaSpillCountStride] (may be null) the query's spill counter is ZEROED once this selection has
                               // read what it needs: the next scan stage appends from 0 again — no memset launch between the stages
    const float* delta;        // [nq] error bound; < 0 = query is skipped (tau = +inf, overflow set)
    float* tau_out;            // [nq] (may be null)
    u64* pool_out;             // [nq, kSelectPool] candidates, kEmpty padded (may be null)
    uint32_t* cand_counts;     // [nq] number of candidates, unclamped (may be null)
    uint32_t* overflow;        // [nq] set when there are more than kSelectPool candidates
    uint32_t take_topk;        // != 0: the candidates are the k best entries themselves (exact pass-1 scores)
    // threshold step with the finish fields set and anchor_unit != null (int8 filter): the candidates are re-scored exactly and
    // tau_out = max(a_k - 2 delta, S_k * anchor_unit[q] - delta), S_k = the k-th best EXACT score among them — k real rows score
    // at least S_k, so every true top-k row's approximate score is at least S_k in filter units minus ONE delta
    const float* anchor_unit;  // [nq] filter-score units per exact-score unit (slab scale x query scale); null = off
    // A sample stage whose survivors only ANCHOR the next threshold (the wide main pass visits every row anyway) may emit any
    // subset of rows — k real rows with exact scores bound the final k-th best whichever rows they are: heur_rank != 0 makes
    // tau_out the approximate score at that rank with NO margin (a few dozen rows of the next, larger sample pass instead of
    // thousands), tau_floor_out keeps the proven threshold, and the next selection falls back to it (tau_floor_in) when fewer
    // than k rows came through
    uint32_t heur_rank;
    float* tau_floor_out;      // [nq] (may be null)
    const float* tau_floor_in; // [nq] (may be null)
    uint32_t big_pool;         // finish step: re-score up to 8,192 candidates per query (sorted variant) instead of kSelectPool
    uint32_t* pool_flag;       // [nq] device memory (may be null).  big_pool == 0: a query with more than kSelectPool candidates
                               // sets its flag INSTEAD of `overflow`; big_pool != 0: only flagged queries are processed (second
                               // chance of the finish, launched right behind the first over the same lists)
    // finish step
    const void* slab;          // [nrows, dim] f16 (f32 when slab_f32 != 0)
    const float* queries;      // [nq, q_stride_f] f32 (the first dim of each are used)
    uint32_t dim, nrows, row_base;
    uint32_t row_stride;       // bytes between slab rows; 0 = dim * 2 (slab_f32: dense rows only, 0 or dim * 4)
    uint32_t query_stride;     // floats between queries; 0 = dim
    int hreduce;
    uint32_t k_out, out_stride;
    uint32_t* out_rows;        // [nq, out_stride] (may be null; 0xffffffff padding)
    float* out_scores;         // [nq, out_stride] (may be null)
    u64* out_packed;           // [nq, out_stride] (may be null; kEmpty padding)
    uint32_t* out_counts;      // [nq] (may be null)
    // finish step with take_topk (the two-pass searches): the k candidates themselves, for a row-sharded index whose root
    // repeats the selection over all shards' candidates — position i of both lists is the same row: its pass-1 entry
    // (integer score as f32 bits) and its exact entry; kEmpty beyond the candidates.  [nq, k] each, may be null.
    u64* cand_approx_out;
    u64* cand_exact_out;
    uint32_t cand_out_stride;  // entries between queries in both (>= k)
    uint32_t valid_queries;       // blocks q >= this are padding slots whose query lies past the caller's array (0 = every block's query exists)
    uint32_t slab_f32;            // != 0: `slab` holds raw f32 rows (Quantization::F32), re-scored in dot_product_f32_bytes_f32's order
    unsigned long long* stamps;   // lab builds (FSGPU_EXPERIMENTS): shader clocks of block 0's phases; null otherwise
};
// select_groups_kernel (mfma_scan.hip): the selection behind a group-maxima sample (MfmaScanArgs::stage == 3).  Per query: the
// kGroupsTaken best of its nentries groups (packed best approximate score | first row of the group's 8 rows: rows g + {0..3} and
// g + 16 + {0..3}) -> their live, allowed rows re-scored from the f16 slab in the reference's operation order -> S_k = the k-th best
// exact score among them (k distinct real rows: a lower bound on the final k-th best) ->
//   tau_out = max(a_k - 2 delta, S_k * anchor_unit - delta) in filter units (a_k: the k-th best group maximum),
// exactly what select_kernel's exact-anchor step emits; the query's spill counter is reset for the scan stage that follows.
// delta < 0 (padding / zero / non-finite query): tau = +inf and overflow[q] = 1 (the exact path answers it).
struct GroupSelectArgs {
    const u64* groups;         // [nq][nentries]
    uint32_t nentries;         // <= 1024
    uint32_t k;                // 1..64
    const float* delta;        // [nq]
    const float* anchor_unit;  // [nq] filter-score units per exact-score unit
    float* tau_out;            // [nq]
    uint32_t* overflow;        // [nq] (may be null)
    uint32_t* spill_reset;     // [nq * kMfmaSpillCountStride] (may be null)
    const void* slab;          // [nrows, dim] f16 (f32 when slab_f32 != 0)
    const u64* live;           // may be null
    const u64* allow;          // may be null
    const float* queries;      // [nq, query_stride] f32
    uint32_t dim, nrows, row_base, query_stride;
    int hreduce;
    uint32_t valid_queries;    // blocks q >= this are padding slots (0 = every block's query exists)
    uint32_t slab_f32;         // != 0: `slab` holds raw f32 rows (Quantization::F32), re-scored in dot_product_f32_bytes_f32's order
    uint32_t rank_only;        // != 0 (the int8 two-pass, whose pass-1 scores are the reference's own): no re-score — tau_out = the k-th
                               // best group maximum itself (k <= 64, delta = 0: k distinct rows score at least that); slab may be null
};
constexpr uint32_t kGroupsTaken = 24;      // groups whose rows are re-scored for ranks up to 24 (192 rows) ...
constexpr uint32_t kGroupsTakenMax = 32;   // ... and up to 32 (256 rows: the two-tier flow's fetch of 3 x 10)
constexpr uint32_t kGroupsRankMax = 128;   // rank-only form (int8 / 4-bit two-pass: k x multiplier candidates, 3 x 30 = 90)
// (the launchers' predicates: what they refuse with hipErrorInvalidValue before anything is launched; host code, no device needed)
bool select_args_ok(const SelectArgs& args);
bool select_groups_args_ok(const GroupSelectArgs& args);
bool list_cut_args_ok(uint32_t nlists, uint32_t list_len);
bool two_pass_merge_args_ok(uint32_t nshards, uint32_t cc, uint32_t k);
hipError_t launch_select_groups(const GroupSelectArgs& args, int nq, hipStream_t stream);
constexpr uint32_t kSelectPool = 1024;
constexpr uint32_t kSelectMaxK = 128;   // largest rank a selection can anchor on (k, or k * multiplier in int8 mode)
hipError_t launch_select(const SelectArgs& args, int nq, hipStream_t stream);
// out[0] = the largest score at slot list_len - 1 of nlists best-first lists (kEmpty = the list is not full), -inf when no list is full:
// no row outside the lists scores above it (the certified lone-query search, VectorIndex::certified_i8_lone_query)
hipError_t launch_list_cut(const u64* lists, uint32_t nlists, uint32_t list_len, float* out, hipStream_t stream);
// Root of a row-sharded two-pass search (search.rs:514-661 over W shards): per query, the W x cc candidate pairs (pass-1 entry,
// exact entry; shard s's lists [nq][cc] start shard_pitch entries after shard s-1's, kEmpty padded) -> the cc best by the pass-1
// order (integer score desc, row asc: exactly the unsharded candidate set, whose members are each in their own shard's top cc)
// -> the k best of those by the exact order.
hipError_t launch_two_pass_merge(const u64* approx_lists, const u64* exact_lists, uint32_t nshards, uint64_t shard_pitch, uint32_t nq,
                                 uint32_t cc, uint32_t k, uint32_t out_stride, uint32_t* out_rows, float* out_scores, uint32_t* out_counts,
                                 hipStream_t stream);
// bits = 8: quantize_i8_query (scale 127/max when max > 0); bits = 4: pack_4bit_query's levels (scale 7/max when max > 1e-9), one per byte
hipError_t launch_prepare_queries_i8(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, void* qi8, float* delta,
                                     hipStream_t stream, int bits = 8);
// the same quantiser for the int8 FILTER of the exact search: delta = a proven bound on |int8 score - exact score / (row
// scale x query scale)| from the slab statistics of launch_i8_slab_stats (see mfma_scan.hip)
hipError_t launch_prepare_queries_i8_filter(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t q_stride,
                                            const unsigned int* slab_max_bits, const unsigned int* slab_stats, void* qi8,
                                            float* delta, hipStream_t stream, float* unit_out = nullptr, double extra_coeff = 0.0);

constexpr uint32_t kMfmaMaxSlots = 32;           // candidate slots per (block, query) staged in LDS
constexpr uint32_t kMfmaSpillCountStride = 16;  // uint32 counters 64 bytes apart
constexpr uint32_t kWideSlots = 32;               // ... by the register-resident-query main pass (mfma_wide.hip)
bool scan_mfma_supported(int dim);
// mfma_wide.hip: main pass with the queries in registers and the row tiles in an LDS-DMA ring; query_tiles 2 = 256, 3 = 384
// queries per launch; one candidate list of args.slots <= kWideSlots entries per (query, block)
bool scan_wide_supported(int dim, int elem_bytes);
bool scan_wide_group_maxima_supported(int dim, int query_tiles);   // MfmaScanArgs::stage == 3 (int8 rows): see select_groups
int scan_wide_max_query_tiles(int dim, int elem_bytes);  // 3 for f16 rows of 384 dimensions, 5 for their int8 form
hipError_t launch_scan_wide(const MfmaScanArgs& args, int query_tiles, int grid, hipStream_t stream, int* occupancy);
bool scan_wide_barrier_sync();    // FSGPU_WIDE_SYNC=barrier (knobs(), vector_index_batched.cpp): launch_scan_wide's 128-row main pass with a block barrier per tile
uint32_t scan_wide_poll_timeouts();   // mfma_wide.hip: slot waits of the 128-row main pass that gave up (0 unless a wave stopped advancing); the debug census prints it
bool scan_wide_flat_priority();   // FSGPU_WIDE_PRIO=off (knobs(), vector_index_batched.cpp): launch_scan_wide's split loop without priority levels
void note_main_pass_kernel(const char* name);  // remembers the instantiation the last main pass ran (last_main_pass_kernel)
const char* last_main_pass_kernel();  // template instantiation of the last batched main pass launched, as rocprofv3 names it
// shape: see mfma_scan.hip (0 = 64 queries; 1..3 = 128 queries with different row tiling / buffering)
int scan_mfma_waves_per_block(int shape);
int scan_mfma_rows_per_tile(int shape);
int scan_mfma_query_tiles(int shape);
int scan_mfma_max_slots(int shape);  // LDS staging capacity per (query, block)
bool scan_mfma_shape_built(int shape);   // the shape is compiled into THIS build (a shipped build: 0 and 2; shapes 1, 3, 4, 5 are experiments only)
// the 128-query shape the batched planner runs for a requested one (FSGPU_MFMA_SHAPE / FSGPU_MFMA_SHAPE_I8; 0 = none asked for): the
// request when it is a shape of this element size that this build contains, else shape 2
int scan_mfma_planner_shape(int requested, int elem_bytes);
hipError_t launch_scan_mfma(const MfmaScanArgs& args, int shape, int grid, hipStream_t stream, int* occupancy);
hipError_t launch_max_row_norm(const void* slab, uint32_t nrows, uint32_t dim, uint32_t row_stride_bytes, unsigned int* out_bits,
                               hipStream_t stream);
// ... of dense f32 rows (the rotation decision of an F32 slab's filter copy)
hipError_t launch_max_row_norm_f32(const float* rows, uint32_t nrows, uint32_t dim, unsigned int* out_bits, hipStream_t stream);
hipError_t launch_prepare_queries(const float* q, uint32_t nq, uint32_t nq_pad, uint32_t dim, uint32_t q_stride,
                                  const unsigned int* max_norm_bits, void* qh, float* delta, hipStream_t stream);

// int8_kernels.hip
// max_ready: *max_bits_dev already holds the (corpus-wide) max-abs — a sharded index reduces the shards' values first
hipError_t launch_slab_maxabs(const void* slab_f16, size_t n_values, unsigned int* max_bits_dev, hipStream_t stream);
hipError_t launch_quantize_slab_i8(const void* slab_f16, size_t n_values, unsigned int* max_bits_dev, void* out_i8,
                                   hipStream_t stream, bool max_ready = false);
// 4-bit levels (-7..7, the reference's nibble quantiser) one per byte: the batched 4-bit pass 1 reuses the int8 matrix-core kernels
hipError_t launch_quantize_slab_4bit_levels(const void* slab_f16, size_t n_values, unsigned int* max_bits_dev, void* out_i8,
                                            hipStream_t stream, bool max_ready = false);
// bounds on what the int8 slab misses of the f16 slab (int8 filter of the exact batched search): stats_dev[0..4) =
// { f32 bits of max_row sum eps^2, max_row sum |r|, max_row sum r^2, non-finite flag }
hipError_t launch_i8_slab_stats(const void* slab_f16, const void* slab_i8, uint32_t nrows, uint32_t dim,
                                const unsigned int* max_bits_dev, unsigned int* stats_dev, hipStream_t stream);
// the int8 filter's rotated copy (int8_kernels.hip): rows / queries through a fixed orthogonal map in f64, rounded once to f32;
// rt = the map TRANSPOSED, [dim][dim] f64.  _f32: a row with an element that is not finite or above 65,504 comes out as NaN.
hipError_t launch_rotate_rows_f16(const void* rows_f16, uint32_t nrows, uint32_t dim, const double* rt, float* out, hipStream_t stream);
hipError_t launch_rotate_rows_f32(const float* rows, uint32_t nrows, uint32_t row_stride, uint32_t dim, const double* rt, float* out,
                                  hipStream_t stream);
// ... and the quantiser / statistics of launch_quantize_slab_i8 / launch_i8_slab_stats over f32 rows, chunk by chunk: max-abs and
// statistics ACCUMULATE into words the caller zeroed
hipError_t launch_maxabs_f32(const float* v, size_t n, unsigned int* max_bits_dev, hipStream_t stream);
hipError_t launch_quantize_f32_i8(const float* v, size_t n, const unsigned int* max_bits_dev, void* out_i8, hipStream_t stream);
hipError_t launch_i8_stats_f32(const float* rows, const void* rows_i8, uint32_t nrows, uint32_t dim, const unsigned int* max_bits_dev,
                               unsigned int* stats_dev, hipStream_t stream);
bool scan_i8_fused_supported(int dim, int kcap);
// 4-bit two-pass (int8_kernels.hip, BITS = 4)
hipError_t launch_pack_slab_4bit(const void* slab_f16, uint64_t count, uint32_t dim, unsigned int* max_bits_dev,
                                 void* out_4bit, hipStream_t stream, bool max_ready = false);
bool scan_4bit_fused_supported(int dim, int kcap);
hipError_t launch_scan_4bit(const ScanArgs& args, const void* slab_4bit, const void* query_4bit, int kcap, int grid,
                            hipStream_t stream, int* occupancy);
hipError_t launch_score_rows_4bit(const ScanArgs& args, const void* slab_4bit, const void* query_4bit, u64* out_packed,
                                  hipStream_t stream);
hipError_t launch_scan_i8(const ScanArgs& args, const void* slab_i8, const void* query_i8, int kcap, int grid,
                          hipStream_t stream, int* occupancy);
hipError_t launch_score_rows_i8(const ScanArgs& args, const void* slab_i8, const void* query_i8, u64* out_packed,
                                hipStream_t stream);
hipError_t launch_packed_rows(const u64* packed, uint32_t n, uint32_t* rows, hipStream_t stream);
hipError_t launch_pack_hits(const uint32_t* rows, const float* scores, uint32_t n, u64* packed, hipStream_t stream);

// bert_kernels.hip
hipError_t launch_bert_embed_ln(const int32_t* ids, const int32_t* positions, const float* word, const float* pos,
                                const float* type0, const float* lnw, const float* lnb, float* x_f32, void* x_h,
                                int tokens, int hidden, float eps, hipStream_t stream);
hipError_t launch_bert_add_ln(float* x_f32, const float* delta, const float* lnw, const float* lnb, void* x_h, int tokens,
                              int hidden, float eps, hipStream_t stream);
bool bert_gemm_ln_supported(int hidden);
hipError_t launch_bert_gemm_ln(const void* a_h, const void* w_h, const float* bias, float* x_f32, void* x_h,
                               const float* lnw, const float* lnb, int M, int hidden, int K, float eps, hipStream_t stream);
hipError_t launch_bert_gemm(const void* a_h, const void* w_h, const float* bias, float* out_f32, void* out_h, int M,
                            int N, int K, bool gelu_half_out, hipStream_t stream);
hipError_t launch_bert_attention(const float* qkv, const uint32_t* offsets, void* ctx_h, int n_docs, int heads,
                                 int hidden, int max_seq, float scale, hipStream_t stream);
hipError_t launch_bert_attention_h(const void* qkv_h, const uint32_t* offsets, void* ctx_h, int n_docs, int heads,
                                   int hidden, int max_seq, float scale, hipStream_t stream);   // Q, K, V already f16
hipError_t launch_bert_pool(const float* x, const uint32_t* offsets, float* out, int n_docs, int hidden,
                            hipStream_t stream);
hipError_t launch_bert_to_half(const float* src, void* dst, size_t n, hipStream_t stream);

// bert_gemm_w.hip: batch-path linears over weights pre-packed in matrix-core fragment order
hipError_t launch_bert_pack_w(const void* w_h, void* packed_h, int N, int K, hipStream_t stream);
bool bert_gemm_w_supported(int N, int K);
// epilogue 0: f32 output; 1: GELU, f16 output; 2: f16 output
hipError_t launch_bert_gemm_w(const void* a_h, const void* wp, const float* bias, float* out_f32, void* out_h, int M, int N,
                              int K, int epilogue, hipStream_t stream);
bool bert_gemm_ln_w_supported(int hidden, int K);
hipError_t launch_bert_gemm_ln_w(const void* a_h, const void* wp, const float* bias, float* x_f32, void* x_h,
                                 const float* lnw, const float* lnb, int M, int hidden, int K, float eps, hipStream_t stream);
// the whole feed-forward block (up-projection, GELU, down-projection, residual, LayerNorm) in one launch
bool bert_ffn_w_supported(int hidden, int inter);
hipError_t launch_bert_ffn_w(const void* w1p, const float* b1, const void* w2p, const float* b2, float* x_f32, void* x_h,
                             const float* lnw, const float* lnb, int M, int hidden, int inter, float eps, hipStream_t stream);
// everything of a layer after the attention in one launch: output projection + LayerNorm, then the feed-forward block
bool bert_post_attn_w_supported(int hidden, int inter);
hipError_t launch_bert_post_attn_w(const void* ctx_h, const void* w0p, const float* b0, const float* ln0w, const float* ln0b,
                                   const void* w1p, const float* b1, const void* w2p, const float* b2, float* x_f32, void* x_h,
                                   const float* lnw, const float* lnb, int M, int hidden, int inter, float eps,
                                   hipStream_t stream);
// The same two steps in ONE kernel form whatever M is (the 64-row-tile GEMM; the 32-row post-attention block): a row's bits depend on
// the model's shape only, never on how many rows ride along (the cross-encoder's batch invariance, bert_reranker.cpp)
hipError_t launch_bert_gemm_w_fixed(const void* a_h, const void* wp, const float* bias, float* out_f32, void* out_h, int M, int N,
                                    int K, int epilogue, hipStream_t stream);
hipError_t launch_bert_post_attn_w_fixed(const void* ctx_h, const void* w0p, const float* b0, const float* ln0w, const float* ln0b,
                                         const void* w1p, const float* b1, const void* w2p, const float* b2, float* x_f32, void* x_h,
                                         const float* lnw, const float* lnb, int M, int hidden, int inter, float eps,
                                         hipStream_t stream);

// bert_rerank.hip: the cross-encoder's own kernels — typed embeddings, the last layer's [CLS]-query attention, pooler + classifier
bool bert_rerank_supported(int hidden);
hipError_t launch_bert_embed_typed_ln(const int32_t* ids, const int32_t* types, const int32_t* positions, const float* word,
                                      const float* pos, const float* type_emb, const float* lnw, const float* lnb, float* x_f32,
                                      void* x_h, int tokens, int hidden, float eps, hipStream_t stream);
hipError_t launch_bert_cls_attention(const void* qkv_h, const uint32_t* offsets, const float* x, void* ctx_cls_h, float* x_cls,
                                     int n_pairs, int heads, int hidden, float scale, hipStream_t stream);
hipError_t launch_bert_cls_head(const float* x_cls, const float* pool_w, const float* pool_b, const float* cls_w, const float* cls_b,
                                float* logits, float* scores, int n_pairs, int hidden, hipStream_t stream);

// bert_query_kernels.hip: the MiniLM-L6 forward for at most 32 tokens in 25 launches (4 per layer + the pooling), every
// add+LayerNorm riding in the prologue of the GEMM that consumes it.  One argument block serves all stages; a stage reads
// the fields it needs.
struct BertQueryArgs {
    int tokens, n_docs;              // tokens <= 32
    const uint32_t* offsets;         // [n_docs + 1]
    // first stage: embedding gather + LayerNorm instead of the pending add+LayerNorm (ids != null)
    const int32_t* ids;
    const int32_t* positions;
    const float *word, *pos, *type0;
    // pending add+LayerNorm: x = LN(x_in + sum of n_parts slabs of parts ([slab][32][384] f32) + prev_bias)
    const float* x_in;
    float* x_out;                    // the block that owns it stores the normalised rows here (null: nobody does)
    const float* parts;
    int n_parts;
    const float *prev_bias, *lnw, *lnb;
    float eps, attn_scale;
    // GEMM: A rows from a_h (f16, leading dimension lda) unless the stage has a LayerNorm prologue; W [n, ldw] f16; bias [n]
    const _Float16* a_h;
    int lda;
    const _Float16* w;
    int ldw, n;
    const float* bias;
    float* out_f32;                  // partial slabs [slab][32][n]
    _Float16* out_h;                 // f16 rows [tokens][n]
};
bool bert_query_path_supported(int hidden, int inter, int heads);
hipError_t launch_bert_q_qkv_attn(const BertQueryArgs& a, int heads, hipStream_t stream);
hipError_t launch_bert_q_gemm(const BertQueryArgs& a, int mode, hipStream_t stream);
hipError_t launch_bert_q_pool(const BertQueryArgs& a, float* out, hipStream_t stream);
// the same stages in ONE launch of bert_q_one_launch_blocks() resident blocks with grid-wide barriers between them
int bert_q_one_launch_blocks();
hipError_t launch_bert_q_one_launch(const BertQueryArgs* stages_dev, const unsigned char* kinds_dev, int n_stages, int tokens, int n_docs,
                                    const uint32_t* offsets, const int32_t* ids, const int32_t* positions, float* out,
                                    unsigned int* counter_dev, unsigned int base, unsigned int* status_mapped, hipStream_t stream);

// bert_docs_w.hip: the whole MiniLM-L6 forward of a batch of texts of at most 32 tokens each in ONE launch — a 32-row block
// owns whole texts, so the six layers chain inside the kernel (native.rs:1142-1236)
struct BertDocsLayer {           // device pointers of one encoder layer: fragment-order f16 weights (bert_pack_w_kernel), f32 vectors
    const void *qkv_wp, *ao_wp, *i_wp, *o_wp;
    const float *qkv_b, *ao_b, *ln1_w, *ln1_b, *i_b, *o_b, *ln2_w, *ln2_b;
};
struct BertDocsArgs {
    const uint32_t* offsets;     // [n_docs + 1] text i owns tokens [offsets[i], offsets[i + 1])
    const uint32_t* blk_tok;     // [nblocks + 1] first token of each row block: boundaries on text boundaries, at most 32 apart
    const uint32_t* blk_doc;     // [nblocks + 1] first text of each row block
    const int32_t* row_id;       // [nblocks * 32] token id of each row of each block, -1 = padding row
    const uint32_t* row_meta;    // [nblocks * 32] rows of the block << 16 | position inside its text << 8 | its text's index among
                                 // the block's non-empty texts
    const float *word, *pos, *type0, *emb_lnw, *emb_lnb;
    const BertDocsLayer* layers; // [nlayers], device memory
    int nlayers;
    float eps, attn_scale;
    float* out;                  // [n_docs][hidden] pooled, L2-normalised
    unsigned long long* stamps;  // lab builds (FSGPU_EXPERIMENTS): shader-clock stamps of block 0's phases; null otherwise
};
bool bert_docs_w_supported(int hidden, int inter, int heads);
hipError_t launch_bert_docs_w(const BertDocsArgs& a, uint32_t nblocks, hipStream_t stream);

// bert_int8.hip: the int8 dynamic-quant linears (FSGPU_BERT_LINEAR_INT8_DYNAMIC) — per-output-channel int8 weights packed in
// fragment order, per-row int8 activations, v_mfma_i32_16x16x64_i8, f32 epilogue.  q buffers are int8, s buffers f32 scales.
bool bert_i8_gemm_supported(int N, int K);   // K % 64 == 0 and N % 64 == 0
size_t bert_i8_packed_bytes(int N, int K);
hipError_t launch_bert_i8_pack_w(const float* w, void* wp, float* sw, int N, int K, hipStream_t stream);
hipError_t launch_bert_i8_quant_rows(const float* x, void* q, float* s, int rows, int K, hipStream_t stream);
hipError_t launch_bert_i8_quant_rows_h(const void* x_h, void* q, float* s, int rows, int K, hipStream_t stream);
hipError_t launch_bert_i8_embed_ln_quant(const int32_t* ids, const int32_t* positions, const float* word, const float* pos,
                                         const float* type0, const float* lnw, const float* lnb, float* x, void* q, float* s, int tokens,
                                         int hidden, float eps, hipStream_t stream);
hipError_t launch_bert_i8_add_ln_quant(float* x, const float* delta, const float* lnw, const float* lnb, void* q, float* s, int tokens,
                                       int hidden, float eps, hipStream_t stream);
hipError_t launch_bert_i8_gemm(const void* qa, const float* sa, const void* wp, const float* sw, const float* bias, float* out, int M,
                               int N, int K, bool gelu, hipStream_t stream);

// mmr_kernels.hip: Maximum Marginal Relevance over slab rows, one workgroup per pool (mmr.rs:103-319 in f64, the reference's
// accumulator order).  Pool q owns rows / scores / ovr_index / out_order [offsets[q], offsets[q + 1]).
constexpr uint32_t kMmrMaxPool = 128, kMmrMaxDim = 1024, kMmrMaxElements = 64 * 1024;   // 128 x 384 and 64 x 1,024 both fit
constexpr uint32_t kMmrLdsHeader = kMmrMaxPool * 8;     // the root norms
constexpr uint32_t kMmrLdsBudget = 160 * 1024;
// the pools the kernel answers; a larger one is left to the host restatement (same bits)
__host__ __device__ inline bool mmr_device_pool(uint32_t n, uint32_t dim) {
    return n <= kMmrMaxPool && dim >= 1 && dim <= kMmrMaxDim && n * dim <= kMmrMaxElements;
}
enum : int { kMmrStageLdsF16 = 0, kMmrStageLdsF32 = 1, kMmrStageGlobalF32 = 2 };
struct MmrArgs {
    const void* slab;             // the index's rows (f16 or f32)
    u64 row_base;                 // global id of the slab's first row
    uint32_t row_stride;          // bytes between rows
    uint32_t dim;
    uint32_t slab_f32;
    uint32_t k, candidate_pool;
    double lambda;                // already clamped (MmrConfig::clamped_lambda)
    const uint32_t* rows;         // global row ids (not read where an override is given)
    const uint32_t* offsets;      // [npools + 1]
    const double* scores;
    const int32_t* ovr_index;     // per candidate: >= 0 = its vector is ovr_vectors[index * dim ..] (a WAL entry); nullptr = none
    const float* ovr_vectors;
    uint32_t* out_order;          // indexes into the pool, in selection order
    uint32_t* out_counts;         // [npools]; not written for a pool the kernel leaves to the host
    double* sims;                 // nullptr: the n x n matrix lives in LDS; else pool q's matrix at sims[offsets[q] * sim_pitch]
    uint32_t sim_pitch;
    uint32_t lds_sims_offset;
    float* vec_ws;                // kMmrStageGlobalF32: staged rows, pool q at vec_ws[offsets[q] * vec_stride]
    uint32_t vec_stride;          // elements between staged rows
};
struct MmrPlan {
    int storage = kMmrStageLdsF16;
    uint32_t vec_stride = 0, lds_sims_offset = 0, lds_bytes = 0;
    bool sims_global = false;
};
// max_n: the largest pool of the launch; f32_staging: an f32 slab, or any override vector; want_sims: the caller reads the matrix
MmrPlan mmr_plan(uint32_t max_n, uint32_t dim, bool f32_staging, bool want_sims);
hipError_t launch_mmr(const MmrArgs& args, uint32_t npools, const MmrPlan& plan, hipStream_t stream);

// join_tile.hpp: the transposed exact join's tile, shared by hubness_kernels.hip and knn_update_kernels.hip.  A 16-lane group owns 4
// rows, so a wave owns 16 in LDS; the other side streams past them in LDS chunks of 16 vectors.
constexpr uint32_t kJoinTileRowsPerWave = 16, kJoinTileChunk = 16;

// hubness_kernels.hip: the query-hubness table (hubness.rs:109-138) — per slab row the mean of its k greatest
// dot_product_f32_f32 similarities to a query sample, selected under f32::total_cmp and summed in the canonical order
// (include/fsgpu.h).  A workgroup owns 16 rows per wave in LDS and streams the sample past them in chunks of kHubQueryChunk.
constexpr uint32_t kHubMaxK = 64, kHubMaxDim = 1024, kHubRowsPerWave = kJoinTileRowsPerWave, kHubQueryChunk = kJoinTileChunk;
constexpr uint32_t kHubLaunchRows = 1u << 20;      // rows per launch: no single launch holds a shared card for long
constexpr size_t kHubLdsBudget = 160 * 1024;
struct HubnessArgs {
    const void* slab;         // the index's rows (f16 or f32)
    uint32_t row_stride;      // bytes between rows
    uint32_t dim;
    uint32_t slab_f32;
    uint32_t row0, nrows;     // this launch: slab rows [row0, row0 + nrows)
    const float* queries;     // [nq, dim]
    uint32_t nq;
    uint32_t k;               // min(kq, nq), 1 .. kHubMaxK
    int32_t hreduce;
    float* out;               // [slab rows]
    float* out_topk;          // nullable: [slab rows, k], greatest first
};
hipError_t launch_hubness(const HubnessArgs& args, hipStream_t stream);

// compact_kernels.hip: rewrite_index's vector pass (lib.rs:3003-3045) as a segmented copy.  The host hands over RUNS — maximal
// stretches of surviving consecutive rows, in destination order, covering the new slab without a gap; a run reads the old slab or
// (kCompactFromWal) the block of already encoded WAL rows.  A wave owns a contiguous range of destination bytes, finds its first
// run by one binary search and walks on from there.
constexpr uint32_t kCompactLaunchRows = 1u << 20;     // destination rows per launch: no single launch holds a shared card for long
constexpr uint32_t kCompactWaveBytes = 16 * 1024;     // destination bytes per wave
constexpr uint64_t kCompactFromWal = 1ull << 63;      // in CompactRun::src: the offset is into the WAL block
struct CompactRun {
    uint64_t src;     // byte offset of the run's first row in its source (| kCompactFromWal)
    uint64_t dst;     // byte offset of the run's first row in the new slab
};                    // (a run ends where the next begins; runs[nruns].dst = the new slab's size)
struct CompactArgs {
    const unsigned char* slab;   // the old slab
    const unsigned char* wal;    // WAL rows in slab format, [W, row_bytes]
    unsigned char* out;          // the new slab
    const CompactRun* runs;      // [nruns + 1]
    uint64_t nruns;
    uint64_t dst_begin, dst_end; // this launch's destination bytes
};
hipError_t launch_compact_runs(const CompactArgs& args, bool nt_stores, hipStream_t stream);

// knn_graph_kernels.hip: the two ends of a k-NN graph build step (vector_index_knn.cpp; include/fsgpu.h).  The step in between is
// the batched search itself: the staged block is its query block, the emit kernel reads its hits.
constexpr uint32_t kKnnChunk = 1024;      // source rows per step
constexpr uint32_t kKnnMaxM = 63;         // k = m + 1 stays inside the fused tiers
constexpr uint32_t kKnnPadRow = 0xffffffffu;
struct KnnStageArgs {
    const void* slab;            // the index's rows (f16 or f32)
    uint32_t row_stride;         // bytes between rows
    uint32_t dim;
    uint32_t slab_f32;
    uint32_t row_base;           // added to the local rows in src_out
    const uint32_t* src_local;   // [n] live source rows of this chunk, local (device-visible)
    uint32_t n;
    float* queries;              // out: [n, dim] f32, row i = slab row src_local[i] widened
    uint32_t* src_out;           // out: [n] global source rows
};
hipError_t launch_knn_stage_rows(const KnnStageArgs& args, hipStream_t stream);
struct KnnEmitArgs {
    const uint32_t* hit_rows;    // [n, m + 1] global rows of the searches, best first
    const float* hit_scores;     // [n, m + 1]
    const uint32_t* hit_counts;  // [n]
    const uint32_t* src;         // [n] global source rows
    uint32_t n, m;
    uint32_t* out_rows;          // [n, m], padded with kKnnPadRow
    float* out_sims;             // nullable: [n, m], padded with 0.0f
};
hipError_t launch_knn_emit(const KnnEmitArgs& args, hipStream_t stream);

// knn_update_kernels.hip: carrying a k-NN table across a rewrite or deletes (vector_index_knn_update.cpp; include/fsgpu.h,
// fsgpu_index_update_knn_graph).  All pointers are device memory.  The working table [n, m] holds a row's list as packed
// entries (device_util.hpp: score bits << 32 | LOCAL current row), best first under sortkey, kEmpty past its end.
constexpr uint8_t kKnnUpdDead = 0, kKnnUpdAdded = 1, kKnnUpdClean = 2, kKnnUpdDirty = 3;   // the class byte of a current row
constexpr uint32_t kKnnUpdMaxDim = 1024;           // dimensions the join covers
constexpr uint32_t kKnnUpdBlock = 1024;            // added rows per join launch (one staged f32 block)
constexpr uint32_t kKnnUpdRowsPerWave = kJoinTileRowsPerWave, kKnnUpdChunk = kJoinTileChunk;   // added rows per LDS chunk
constexpr uint32_t kKnnUpdLaunchRows = 1u << 20;   // rows per join launch: no single launch holds a shared card for long
constexpr size_t kKnnUpdLdsBudget = 159 * 1024;   // dynamic LDS of the join; the block vote's static bytes come on top
// fsgpu_knn_update_config_default's max_added_fraction: of the swept 0.1 / 0.3 / 1 / 3 % of added rows at 1M x 384, m = 16, the
// largest at which the update still beat a rebuild was 0.3 % (2.9 x; at 1 % it lost, 0.97 x), halved
constexpr float kKnnUpdDefaultMaxAddedFraction = 0.0015f;
// inv[new_to_old[x]] = x for every x with a predecessor (< old_len); inv was filled with 0xff bytes.  No predecessor occurs twice.
hipError_t launch_knn_update_inverse(const uint32_t* new_to_old, uint64_t n, uint64_t old_len, uint32_t* inv, hipStream_t stream);
struct KnnUpdClassifyArgs {
    const uint32_t* old_rows;    // [old_len, m] global ids relative to old_row_base, kKnnPadRow padding
    const float* old_sims;       // [old_len, m]
    uint64_t old_len;
    uint32_t old_row_base;
    const uint32_t* new_to_old;  // [n] old local row or kKnnPadRow; nullptr = identity (old_len == n)
    const uint32_t* inv;         // [old_len] current row of an old row or kKnnPadRow; nullptr = identity
    const u64* live;             // bit r set = row r live; nullptr = all live
    uint64_t n;                  // current rows
    uint32_t m;
    uint32_t all_dirty;          // != 0: the map is not monotone, every kept row is dirty
    uint8_t* cls;                // out: [n]
    u64* work;                   // out: [n, m] the remapped, sorted list of a kept-clean row; kEmpty everywhere else
};
hipError_t launch_knn_update_classify(const KnnUpdClassifyArgs& args, hipStream_t stream);
struct KnnUpdScatterArgs {       // a search step's lists (knn_emit_kernel's output) into the working table at their sources' rows
    const uint32_t* src;         // [n] global source rows
    const uint32_t* rows;        // [n, m] global ids, kKnnPadRow padding
    const float* sims;           // [n, m]
    uint32_t n, m, row_base;
    uint64_t nrows;              // rows of the working table (every source and id is checked against it)
    u64* work;
};
hipError_t launch_knn_update_scatter(const KnnUpdScatterArgs& args, hipStream_t stream);
struct KnnUpdJoinArgs {
    const void* slab;            // the index's rows (f16 or f32)
    uint32_t row_stride, dim, slab_f32;
    int32_t hreduce;
    uint32_t row0, nrows;        // this launch's rows [row0, row0 + nrows)
    uint32_t m;
    const uint8_t* cls;          // [slab rows]: only kKnnUpdClean rows are scored into
    u64* work;                   // [slab rows, m] in and out
    const float* added;          // [n_added, dim] the added rows widened to f32 (knn_stage_rows_kernel's block)
    const uint32_t* added_rows;  // [n_added] their LOCAL rows
    uint32_t n_added;
};
hipError_t launch_knn_update_join(const KnnUpdJoinArgs& args, hipStream_t stream);
struct KnnUpdOutputArgs {
    const u64* work;             // [n, m]
    const uint8_t* cls;          // [n]
    uint64_t n;
    uint32_t m, row_base;
    uint32_t* out_rows;          // [n, m] global ids, kKnnPadRow padding
    float* out_sims;             // [n, m], 0.0f padding
    uint32_t* join_entries;      // [blocks] per block: entries of kept-clean lists that are added rows (summed by the host)
};
uint32_t knn_update_output_blocks(uint64_t n, uint32_t m);
hipError_t launch_knn_update_output(const KnnUpdOutputArgs& args, hipStream_t stream);

// knn_optimize_kernels.hip: the graph optimisation over a neighbour table (vector_index_knn_optimize.cpp; include/fsgpu.h,
// fsgpu_knn_graph_optimize).  All pointers are device memory; n <= 2^32 - 2, 1 <= degree <= width <= kKnnOptMaxWidth.
constexpr uint32_t kKnnOptMaxWidth = 64;   // a list is one wave wide
struct KnnOptDetourArgs {
    const uint32_t* table;       // [n, width] global ids, kKnnPadRow ends a list (the caller's: every id is checked against n)
    uint64_t n;
    uint32_t width, degree, row_base;
    uint32_t* fwd;               // out: [n, degree] F(x) as global ids, dense, then kKnnPadRow
    uint32_t* max_detour;        // nullable: [1], raised to the greatest detour count
    uint8_t* seen_before;        // nullable: [n], 1 where an edge of the table's first `degree` columns points
};
hipError_t launch_knn_opt_detour(const KnnOptDetourArgs& args, hipStream_t stream);
struct KnnOptRoundArgs {         // the reverse candidates of one rank, placed in (source ascending) order behind the ranks before it
    const uint32_t* fwd;         // [n, degree]
    uint64_t n;
    uint32_t degree, rank, row_base;
    u64* keys;                   // [n] scratch: the round's keys
    u64* sorted;                 // [n] scratch: ... sorted (not `keys`)
    uint32_t* advance;           // [n] scratch
    uint32_t* fill;              // [n] candidates placed per target so far (0 before rank 0), capped at degree
    uint32_t* rev;               // [n, degree] the candidates as global ids; only the first fill[y] of a row are written
};
hipError_t launch_knn_opt_round(const KnnOptRoundArgs& args, void* sort_temp, size_t sort_temp_bytes, hipStream_t stream);
struct KnnOptMergeArgs {
    const uint32_t* fwd;         // [n, degree]
    const uint32_t* rev;         // [n, degree]
    const uint32_t* fill;        // [n]
    uint64_t n;
    uint32_t degree, row_base;
    uint32_t* out;               // [n, degree] global ids, dense, then kKnnPadRow
    u64* edge_counts;            // nullable: [2] += entries written from F, from the reverse candidates
    uint8_t* seen_after;         // nullable: [n], 1 where an edge of `out` points
};
hipError_t launch_knn_opt_merge(const KnnOptMergeArgs& args, hipStream_t stream);
// out2[0] += rows with before[i] == 0, out2[1] += rows with after[i] == 0
hipError_t launch_knn_opt_count_zero(const uint8_t* before, const uint8_t* after, uint64_t n, u64* out2, hipStream_t stream);

// ann_kernels.hip: the beam search over a k-NN table (ann_index.cpp; include/fsgpu.h, "graph ANN search").  One
// workgroup per query; everything of a query but its slab rows lives in LDS.
constexpr uint32_t kAnnMaxEf = 256;             // beam entries
constexpr uint32_t kAnnMaxExpand = 8;
constexpr uint32_t kAnnMaxStepRows = 512;       // expand * degree: the rows one step can walk
constexpr uint32_t kAnnMaxAdmitted = 4096;      // max_iters * expand * degree: the rows the steps of a query can admit ...
constexpr uint32_t kAnnTableSlots = 8192;       // ... into an open-addressing table that stays at most half full
constexpr uint32_t kAnnMaxEntry = 65536;        // entry rows (they do not occupy the table)
constexpr uint32_t kAnnMaxDim = 16384;          // the query sits in LDS as f32
struct AnnSearchArgs {
    const void* slab;            // the index's rows (f16 or f32)
    const u64* live;             // bit r set = row r live; nullptr = all live
    const uint32_t* graph;       // [nrows, width] global row ids, kKnnPadRow ends a list (device)
    const float* queries;        // [nq, dim] f32 (device)
    uint32_t nrows, dim, row_base, row_stride, slab_f32;
    int32_t hreduce;
    uint32_t width, degree, expand, max_iters, n_entry;   // 1 <= degree <= width, n_entry <= nrows
    uint32_t k, ef;              // 1 <= k <= ef <= kAnnMaxEf
    uint32_t* out_rows;          // [nq, k] global rows, best first; kKnnPadRow past the count
    float* out_scores;           // [nq, k]; 0.0f past the count
    uint32_t* out_counts;        // [nq]
    uint32_t* out_scored;        // [nq] rows scored (entry rows and admitted rows)
    uint32_t* out_steps;         // [nq] steps taken
};
bool ann_args_ok(const AnnSearchArgs& args);   // what the launcher refuses with hipErrorInvalidValue (host code, no device needed)
size_t ann_lds_bytes(uint32_t dim);
hipError_t launch_ann_search(const AnnSearchArgs& args, uint32_t nq, hipStream_t stream);

// search_hits_kernels.hip: the WAL half and the resolve step of the batched search_hits (vector_index_hits.cpp)
constexpr uint32_t kHitsMaxK = 256;
struct WalTopkArgs {
    const float* wal;        // [W, dim] f32 mirror of the resident WAL embeddings
    const float* queries;    // [nq, dim] f32
    uint32_t nq, W, dim;
    uint32_t kw;             // entries kept per query: min(k, W), 1 .. kHitsMaxK
    uint32_t nrows;          // WAL entry w is packed as (score, nrows + w): it sorts behind every main row of equal score
    int32_t hreduce;         // FSGPU_HREDUCE_*
    u64* out_packed;         // nullable: [nq, kw] best first, kEmpty padded; non-finite scores are skipped (search.rs:1466-1470)
    float* out_scores;       // nullable (lab): [nq, W] every score as computed
};
// false: one query of this dimension and its candidate buffers do not fit the LDS (the caller takes the per-query path)
bool wal_topk_supported(uint32_t dim, uint32_t kw);
hipError_t launch_wal_topk(const WalTopkArgs& args, hipStream_t stream);
struct ResolveHitsArgs {
    const uint32_t* main_rows;    // [nq, k] best first (the batched search's device output)
    const float* main_scores;     // [nq, k]
    const uint32_t* main_counts;  // [nq]
    const u64* wal_packed;        // [nq, kw]; unused when kw == 0
    const u64* live;              // nullable: bit r set = main row r live
    const u64* shadowed;          // nullable: bit r set = main row r's doc id has a resident WAL entry
    const uint32_t* main_class;   // [nrows] doc-id class of a main row: the first row with the same id bytes
    const uint32_t* wal_class;    // [W] ... of a WAL entry: its main row's class, else nrows + the first WAL index with the id
    uint32_t nq, k, kw, nrows;
    uint32_t* out_rows;           // [nq, k] compacted, zero padded
    float* out_scores;            // [nq, k]
    uint32_t* out_counts;         // [nq]
};
hipError_t launch_resolve_hits(const ResolveHitsArgs& args, hipStream_t stream);

// index_build_kernels.hip: the two device passes of the index builder (index_builder.cpp).  Staged rows live in chunks of
// chunk_rows rows behind a device table of chunk pointers: staged position p is row p % chunk_rows of chunks[p / chunk_rows].
constexpr uint32_t kBuildLaunchRows = 1u << 20;    // rows per launch: no single launch holds a shared card for long
constexpr uint32_t kBuildTileRows = 64;            // ingest: rows per wave, one per lane
constexpr uint32_t kBuildTileCols = 64;            // ingest: columns per LDS tile
constexpr u64 kBuildVerdictNone = ~0ull;           // IngestArgs::verdict when every row passed
constexpr uint32_t kBuildNonFinite = 1, kBuildBadNorm = 2;   // low byte of the verdict word: which rule the row broke
struct IngestArgs {
    const float* src;              // [n, dim] f32 rows of this launch
    unsigned char* const* chunks;  // the staging chunks
    uint32_t chunk_rows;
    uint32_t dim;
    uint32_t n;                    // rows of this launch, <= kBuildLaunchRows and n * dim < 2^31
    uint32_t to_f16;               // 1: rows are staged as round-to-nearest-even f16; 0: as raw f32
    u64 first_pos;                 // staged position of row 0
    u64 first_row;                 // index of row 0 in its add call (for the verdict)
    u64* verdict;                  // atomicMin of (row in call << 8 | rule) over the offending rows
};
hipError_t launch_build_ingest(const IngestArgs& args, hipStream_t stream);
struct PermuteArgs {
    unsigned char* const* chunks;  // the staging chunks
    uint32_t chunk_rows;
    uint32_t row_bytes;            // 2 .. : dim * 2 or dim * 4
    const uint32_t* perm;          // [slab rows]: staged position of every slab row
    unsigned char* out;            // the slab in file order
    u64 row_begin, row_end;        // this launch's slab rows
};
hipError_t launch_build_permute(const PermuteArgs& args, hipStream_t stream);

// filter_gather_kernels.hip: a filter per query in one batched call (vector_index_filtered.cpp)
// The ascending local row ids of the set bits of an allow bitmap (bits past nrows ignored), built on the device: popcount per word,
// exclusive scan, expand.  scratch: filter_row_list_scratch_bytes(nrows); out_rows holds cap entries (the bitmap's popcount);
// *out_total (device) = the rows written.
constexpr uint32_t kRowListWordsPerBlock = 1024;
size_t filter_row_list_scratch_bytes(uint32_t nrows);
hipError_t launch_filter_row_list(const u64* words_dev, uint32_t nrows, uint32_t cap, uint32_t* scratch, uint32_t* out_rows,
                                  uint32_t* out_total, hipStream_t stream);
// The segmented gather scan: group g = the queries [q0, q0 + nq) of args.queries that share one selective filter, whose row list is
// rows[0 .. n).  One launch, grid (grid_x, groups): nblocks <= grid_x blocks of a group walk its 64-row tiles; every (query, block
// < grid_x) owns one best-first list of k packed entries in partial — [query slot][grid_x][list_stride], kEmpty padded — for
// merge_topk_kernel.
constexpr uint32_t kGatherTileRows = 64;
constexpr uint32_t kGatherMaxK = 256;
constexpr size_t kGatherLdsBudget = 160 * 1024;
struct FilterGatherGroup {
    const uint32_t* rows;   // ascending local row ids (device)
    uint32_t n;             // rows in the list
    uint32_t q0, nq;        // the group's query slots
    uint32_t nblocks;       // blocks that share the group's tiles
};
struct FilterGatherArgs {
    const void* slab;                  // [nrows, dim] f16, rows row_stride bytes apart
    const u64* live;                   // bit r set = row r live; nullptr = all live.  Tested when a row is staged.
    const float* queries;              // [slots, dim] f32, in group order
    const FilterGatherGroup* groups;   // [gridDim.y] (device)
    u64* partial;                      // [slots, grid_x, list_stride]: the first k entries of a list are its result
    uint32_t list_stride;              // >= k, and >= 64 for k <= 64 (between tiles a block parks one entry per lane there)
    uint32_t nrows, dim, k, row_base, row_stride;
    int32_t hreduce;
};
bool filter_gather_supported(uint32_t dim, uint32_t k);   // dim % 8 == 0, k <= kGatherMaxK, a tile of this dimension fits the LDS
hipError_t launch_filter_gather_scan(const FilterGatherArgs& args, uint32_t ngroups, uint32_t grid_x, hipStream_t stream);

// ivf_kernels.hip: the inverted-file index (ivf_index.cpp; include/fsgpu.h, "IVF index").  All pointers are device
// memory.  The probed lists are scanned by launch_filter_gather_scan as it is: a probed list is a FilterGatherGroup.
constexpr uint32_t kIvfMaxLists = 65536, kIvfMaxProbe = 256, kIvfMaxIters = 64;
constexpr uint32_t kIvfMergeMaxEntries = 16384;   // nprobe * k: what the per-query merge sorts in LDS in one pass
constexpr uint32_t kIvfNoSlot = 0xffffffffu;      // a (query, probed list) pair whose list is empty owns no slot
constexpr uint32_t kIvfLaunchRows = 1u << 20;     // rows per assignment launch: no single launch holds a shared card for long
constexpr size_t kIvfLdsBudget = 159 * 1024;      // dynamic LDS of the assignment; the block vote's static bytes come on top
// Assignment, the third user of join_tile.hpp: slab rows in LDS, the centroids streamed past them, per row a running list of ONE
// entry keyed (score_ord << 32 | ~centroid) — score descending with NaN as -inf, the lower centroid first.  The score is
// dot_product_f16_bytes_f32(row, centroid) in the hreduce order: fsgpu_gather_dot's bits.
struct IvfAssignArgs {
    const void* slab;            // the index's f16 rows
    uint32_t row_stride, dim;
    int32_t hreduce;
    uint32_t row0, nrows;        // this launch's rows [row0, row0 + nrows)
    const u64* gate;             // bit r set = row r is assigned; nullptr = every row
    const float* centroids;      // [nlist, dim]
    uint32_t nlist;
    uint32_t* assign;            // [slab rows]; a row outside the gate is not written
};
bool ivf_assign_supported(uint32_t dim);   // the tile of one wave fits the LDS
hipError_t launch_ivf_assign(const IvfAssignArgs& args, hipStream_t stream);
// rows r < n with gate bit set and assign[r] != prev[r], added to *out (an integer sum: no order reaches it)
hipError_t launch_ivf_count_changed(const uint32_t* assign, const uint32_t* prev, const u64* gate, uint32_t n, u64* out, hipStream_t stream);
// Lists from assign[n] (>= nlist: in no list): keys (nlist - list) << 32 | ~row sorted descending by the library's radix sort, i.e.
// ascending (list, row), then offsets [nlist + 1] from the list boundaries of the sorted keys and rows [offsets[nlist]].  No atomics.
// keys, sorted: [n] scratch; sort_temp: sort_keys_desc_temp_bytes(n).
hipError_t launch_ivf_lists(const uint32_t* assign, uint32_t n, uint32_t nlist, u64* keys, u64* sorted, void* sort_temp, size_t sort_temp_bytes,
                            u64* offsets, uint32_t* rows, hipStream_t stream);
// Centroid update: per list with members and per dimension the f64 sum of the widened values SEQUENTIAL in ascending row order, the
// f64 mean, norm2 = the sequential f64 sum over ascending d of mean_d * mean_d (a multiply and an add), and, when norm2 is finite and
// > 0, centroid_d = (float)(mean_d / sqrt(norm2)); otherwise, and for a list without members, the centroid stays.
struct IvfUpdateArgs {
    const void* slab;
    uint32_t row_stride, dim;
    const uint32_t* list_rows;
    const u64* offsets;          // [nlist + 1]
    uint32_t nlist;
    float* centroids;            // [nlist, dim] in and out
};
hipError_t launch_ivf_update(const IvfUpdateArgs& args, hipStream_t stream);
// Per-query merge: query q reads the best-first lists (k packed entries each, kEmpty behind the entries) of its nprobe slots and
// writes its best k — rows, scores, count — under sortkey.  nprobe * k <= kIvfMergeMaxEntries.
struct IvfMergeArgs {
    const u64* slot_lists;       // slot s at slot_lists + s * slot_stride
    uint64_t slot_stride;
    const uint32_t* qslots;      // [nq, nprobe] slot or kIvfNoSlot
    uint32_t nprobe, k;
    uint32_t* out_rows;          // [nq, k], 0xffffffff past the count
    float* out_scores;           // [nq, k]
    uint32_t* out_counts;        // [nq]
};
hipError_t launch_ivf_merge(const IvfMergeArgs& args, uint32_t nq, hipStream_t stream);

// ivf_filter_kernels.hip: the int8 matrix-core list filter (ivf_index.cpp; ivf_filter_plan.hpp).  The caps of the filter
// (mirrored in tests/ivf_filter_cases.py, reported by fsgpu_ivf_filter_stats):
constexpr uint32_t kIvfFilterKCap = 64;          // k above it: the whole call takes the unfiltered path
constexpr uint32_t kIvfFilterSlotCap = 128;      // candidates a slot may keep; more: the slot overflows and is scanned whole
constexpr uint64_t kIvfFilterScratchEntries = 1ull << 26;   // int32 scores resident at once (256 MB); a call above it runs in ranges of tiles
constexpr uint32_t kIvfFilterTileQueries = 16;   // member queries of a list per work item: one MFMA column tile
constexpr uint32_t kIvfFilterRowTile = 16;       // list starts of the ordered copy are aligned to it: one MFMA row tile
constexpr uint32_t kIvfFilterItemRows = 512;     // rows a workgroup scores for its tile: 8 row tiles per wave
constexpr uint32_t kIvfFilterPitchAlign = 64;    // row pitch of the ordered copy: one MFMA k-step, zero padded
constexpr int32_t kIvfFilterDead = INT32_MIN;    // the integer score of a dead row and of the padding rows: below every real score
constexpr uint32_t kIvfFilterFlagOverflow = 1, kIvfFilterFlagUncertified = 2, kIvfFilterFlagAboveScratch = 4;
// ordered[list start of l, padded to kIvfFilterRowTile rows, + i][0 .. dim) = filter_i8[list_rows[offsets[l] + i]][0 .. dim); the
// bytes dim .. pitch of a row and the padding rows are zero.  pad_row0: [nlist] the first ordered row of each list.
hipError_t launch_ivf_filter_gather(const signed char* filter_i8, uint32_t dim, const uint32_t* list_rows, const u64* offsets, const u64* pad_row0,
                                    uint32_t nlist, uint64_t total, uint32_t pitch, signed char* ordered, hipStream_t stream);
// A tile: up to kIvfFilterTileQueries consecutive slots of one list.  Slot slot0 + j keeps s[i], i < len_pad = len rounded up to
// kIvfFilterRowTile, at scores + scratch0 + j * len_pad: the int32 dot of the query's codes with row i's, kIvfFilterDead for a dead row
// and for i >= len.  Workgroup w of the launch serves the tile t with item0[t] <= item_first + w < item0[t + 1], rows from
// (item_first + w - item0[t]) * kIvfFilterItemRows on.  (IvfFilterTile: ivf_filter_tile.hpp, which the host plan shares.)
struct IvfFilterScoreArgs {
    const signed char* ordered;
    uint32_t pitch;                 // bytes, a multiple of kIvfFilterPitchAlign
    const signed char* codes;       // [nq, dim] the queries' int8 codes
    uint32_t dim;
    const uint32_t* slot_query;     // [slots]
    const uint32_t* list_rows;
    const u64* live;                // as it is now; nullptr = all live
    const IvfFilterTile* tiles;     // [ntiles + 1]: the last entry carries the end of the items
    uint32_t tile_first, ntiles, item_first;   // this launch's tiles and the first item among them
    int32_t* scores;
};
hipError_t launch_ivf_filter_score(const IvfFilterScoreArgs& args, uint32_t nitems, hipStream_t stream);
// One workgroup per slot: the k-th largest score t with multiplicity (kIvfFilterDead when no more than k rows are live), the margin
// m = ceil(2 delta) of the slot's query, and the list_rows entries of the live rows with s >= t - m (every live row when no more than
// k are), ascending, the first kIvfFilterSlotCap of them at cand + slot * kIvfFilterSlotCap; count is never clipped.
// flag: kIvfFilterFlagOverflow | kIvfFilterFlagUncertified (delta < 0: nothing else is written for the slot but count 0).
struct IvfFilterSelectArgs {
    const int32_t* scores;
    const IvfFilterTile* tiles;
    const uint32_t* slot_tile;      // [slots] the tile of a slot
    const uint32_t* slot_query;
    const float* delta;             // [nq]
    const uint32_t* list_rows;
    uint32_t slot_first, k;
    int32_t* out_t;                 // [slots]
    long long* out_m;               // [slots]
    uint32_t* out_count;            // [slots]
    uint32_t* out_flag;             // [slots]
    uint32_t* cand;                 // [slots, kIvfFilterSlotCap]
};
hipError_t launch_ivf_filter_select(const IvfFilterSelectArgs& args, uint32_t nslots, hipStream_t stream);

}  // namespace fsgpu

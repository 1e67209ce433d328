/* fsgpu_lab.h — entry points of libfsgpu.so that exist for bench.py, the profiling scripts and A/B runs; NOT part of the drop-in
 * boundary (include/fsgpu.h), no reference interface behind them.  A host that embeds the library never needs this header.
 */
#ifndef FSGPU_LAB_H
#define FSGPU_LAB_H

#include "fsgpu.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- bench / test fixture ---- */
/* The reference's own bench generator (frankensearch/benches/fsvi_4bit_vs_incumbent.rs:56-101,344-365) run on the GPU so that
 * a 10M- or 50M-row corpus never crosses PCIe: xorshift64 raw_vector, `clusters` normalised centroids
 * (seed 0xc0000000 + c), vector i = normalize(centroid[i % clusters] + noise * raw_vector(seed_base + i)) for
 * i in [first, first + n).  as_f16 = 1: out_dev receives n x dim little-endian f16 rows (corpus: seed_base 1);
 * as_f16 = 0: n x dim f32 (queries: seed_base 0xdead0000).  The bytes equal the CPU generator's (same operation order).
 * hip_stream may be NULL (default stream); the call returns after the kernels have finished. */
fsgpu_status fsgpu_bench_fixture_device(int32_t device, uint64_t first, uint64_t n, uint32_t dim, uint32_t clusters, float noise,
                                        uint64_t seed_base, int32_t as_f16, void *out_dev, void *hip_stream);

/* ---- instrumentation ---- */
/* When enabled, HIP events bracket the scan kernel of every fsgpu_search_topk* call; enabled = n > 1: of the batched exact search's
 * merged main launch only every n-th is bracketed (an event pair idles the stream ~6 us on either side of the launch). */
fsgpu_status fsgpu_index_set_profiling(fsgpu_index *idx, int32_t enabled);
/* Sum of scan-kernel time (ms) and number of scan launches since the last reset; synchronises. */
fsgpu_status fsgpu_index_scan_time(fsgpu_index *idx, double *total_ms, uint64_t *launches, int32_t reset);
/* Same, plus the number of slab rows those launches streamed (the batched path's timed main pass skips the rows its
 * sampling stage already covered), so that bytes/launch can be stated exactly. */
fsgpu_status fsgpu_index_scan_stats(fsgpu_index *idx, double *total_ms, uint64_t *launches, uint64_t *rows,
                                    int32_t reset);
/* Filtered searches (allow bitmap given) answered by scoring only the allowed rows (try_gather_filtered,
 * crates/frankensearch-index/src/search.rs:1114-1180: taken when allowed * 50 < rows) and by the masked full scan. */
fsgpu_status fsgpu_index_filter_stats(fsgpu_index *idx, uint64_t *gathered, uint64_t *scanned);
/* The grouping and path decision of fsgpu_search_topk_batched_multi_filtered on its own, host code only (no device is looked for):
 * groups are numbered in the order their first query appears, no filter (-1) is a group like any other, a filter no query names
 * forms none.  out_group_of_query [nq]; out_path_of_group [*out_ngroups <= nfilters + 1]: 0 unfiltered, 1 dense (allowed * 50 >=
 * nrows), 2 gather (0 < allowed * 50 < nrows), 3 empty (allowed == 0).  An entry < -1 or >= nfilters: FSGPU_ERR_INVALID_CONFIG. */
fsgpu_status fsgpu_lab_multi_filter_plan(uint64_t nrows, const uint64_t *allowed_per_filter, uint32_t nfilters,
                                         const int32_t *filter_of_query, uint32_t nq, int32_t *out_group_of_query,
                                         int32_t *out_path_of_group, uint32_t *out_ngroups);
/* Name of the template instantiation the last batched main pass launched in this process ran ("" before the first one), spelled as
 * rocprofv3 prints it: lets bench.py tie a committed PMC summary to the kernel that actually ran. */
const char *fsgpu_last_main_pass_kernel(void);
/* The library's own descending radix sort of 64-bit sortkeys (csrc/sort_general.hip: the collect-all / large-k path,
 * search.rs:449-473), host arrays in and out — so that tests can check it against a host sort at tile boundaries.  varying_bits: the
 * bits in which two keys of the input may differ (~0 when unknown): a digit without one gets no pass. */
fsgpu_status fsgpu_lab_sort_keys_desc(int32_t device, const uint64_t *keys, uint64_t n, uint64_t varying_bits, uint64_t *out_sorted);
/* The int8 dynamic-quant linear of FSGPU_BERT_LINEAR_INT8_DYNAMIC on host buffers, for kernel-level tests: W [N, K] f32 through the
 * load-time weight packer, x [M, K] f32 through the row quantiser, then the int8 GEMM with the bias epilogue: y [M, N] f32.
 * K and N must be multiples of 64 (else FSGPU_ERR_INVALID_CONFIG). */
fsgpu_status fsgpu_lab_linear_int8_dynamic(int32_t device, const float *x, const float *w, const float *bias, uint32_t m, uint32_t n,
                                           uint32_t k, float *y);
/* ONE stage of the f16 encoder (or of the cross-encoder built on it) on host arrays, through the launch_bert_* function the product
 * calls, so that the kernel a shape selects is the product's choice: for kernel-level tests against a high-precision reference
 * (tests/encoder_stage_ref.py).  f32 host inputs the product holds as f16 (activations `a`, contexts, Q/K/V of the f16 attention,
 * weight matrices) are rounded on the device (RNE) and weights of the packed forms re-laid in fragment order, as at model load; f16
 * outputs come back widened to f32.  max_seq is derived from `offsets` as embed_batch does.  A shape a launcher's own *_supported
 * predicate refuses is FSGPU_ERR_INVALID_CONFIG and nothing is launched.  Every output buffer lies between two guard bands of 64
 * rows of a fixed pattern: FSGPU_ERR_DEVICE ("guard band") if a kernel wrote into one.  in[] / out0 / out1 by stage and form:
 *   ATTENTION   in: qkv [m, 3 hidden] (Q | K | V), form 2 also x [m, hidden]; offsets [n_docs + 1] (documents of <= 512 tokens);
 *               forms 0 launch_bert_attention_h, 1 launch_bert_attention: out0 = ctx [m, hidden];
 *               form 2 launch_bert_cls_attention (no empty document): out0 = ctx_cls [n_docs, hidden], out1 = x_cls [n_docs, hidden]
 *   LINEAR      in: a [m, k], w [n, k], bias [n]; out0 = y [m, n].  form 0 launch_bert_gemm (epilogue 0 f32, 1 GELU f16),
 *               1 launch_bert_gemm_w, 2 launch_bert_gemm_w_fixed (epilogue 0 f32, 1 GELU f16, 2 f16)
 *   LINEAR_LN   x = LayerNorm(x + a w^T + bias): in: a [m, k], w [hidden, k], bias, x [m, hidden], ln_w, ln_b; out0 = x (f32), out1 = its
 *               f16 copy.  form 0 launch_bert_gemm_ln, 1 launch_bert_gemm_ln_w, 2 launch_bert_gemm then launch_bert_add_ln
 *   POST_ATTN   everything of a layer after the attention: in: ctx [m, hidden], w0 [hidden, hidden], b0, ln0_w, ln0_b, w1 [inter, hidden],
 *               b1, w2 [hidden, inter], b2, ln_w, ln_b, x [m, hidden]; out0 / out1 as LINEAR_LN.  form 0 launch_bert_post_attn_w,
 *               1 launch_bert_post_attn_w_fixed, 2 launch_bert_gemm_ln_w then launch_bert_ffn_w
 *   EMBED_LN    in: word [vocab, hidden], pos [max_pos, hidden], type [1 | 2, hidden], ln_w, ln_b; ids, positions (, types) [m];
 *               form 0 launch_bert_embed_ln, 1 launch_bert_embed_typed_ln; out0 / out1 as LINEAR_LN
 *   POOL        in: x [m, hidden]; offsets; launch_bert_pool: out0 = [n_docs, hidden]
 *   CLS_HEAD    the cross-encoder's head, launch_bert_cls_head over m pairs: in: x_cls [m, hidden], pool_w [hidden, hidden], pool_b [hidden],
 *               cls_w [hidden], cls_b [1]; out0 = logits [m], out1 = scores [m].  hidden as bert_rerank_supported has it (a multiple of 64,
 *               <= 1024) */
#define FSGPU_LAB_BERT_ATTENTION 0
#define FSGPU_LAB_BERT_LINEAR 1
#define FSGPU_LAB_BERT_LINEAR_LN 2
#define FSGPU_LAB_BERT_POST_ATTN 3
#define FSGPU_LAB_BERT_EMBED_LN 4
#define FSGPU_LAB_BERT_POOL 5
#define FSGPU_LAB_BERT_CLS_HEAD 6
typedef struct fsgpu_lab_bert_stage_args {
    uint32_t stage, form, epilogue;
    uint32_t m, n, k, hidden, inter, n_docs, vocab, max_pos;
    float eps, scale;
    const uint32_t *offsets;
    const int32_t *ids, *positions, *types;
    const float *in[12];
    float *out0, *out1;
} fsgpu_lab_bert_stage_args;
fsgpu_status fsgpu_lab_bert_stage(int32_t device, const fsgpu_lab_bert_stage_args *args);
/* ONE launch of the encoder's int8 dynamic-quant mode (bert_int8.hip) on host arrays, through the launch_bert_i8_* function
 * NativeEmbedder::forward_int8 calls: for kernel-level tests against tests/int8_stage_ref.py.  int8 codes cross the boundary as they are
 * (one byte each), f32 as they are.  Shapes are the launchers' own: n and k multiples of 64, hidden a multiple of 64 and <= 1024; k is
 * capped at 4096 here (127 x 127 x k must stay below 2^31: the accumulator is i32); anything else is FSGPU_ERR_INVALID_CONFIG with nothing
 * launched.  Arguments are checked before a device is looked for.  Every output lies between guard bands as for fsgpu_lab_bert_stage.
 *   QUANT_ROWS     in: x [m, k].  form 0 launch_bert_i8_quant_rows (f32 rows); form 1 launch_bert_i8_quant_rows_h: x is rounded to f16 on
 *                  the device (launch_bert_to_half) first.  out_codes [m, k], out_scales [m]
 *   PACK_W         launch_bert_i8_pack_w.  in: w [n, k]; out_codes = the n k packed bytes in fragment order, out_scales = sw [n]
 *   GEMM           launch_bert_i8_pack_w then launch_bert_i8_gemm.  codes [m, k] (the activation codes, given directly), in: sa [m],
 *                  w [n, k], bias [n]; epilogue 0 bias, 1 bias + GELU; out_f32 = y [m, n]
 *   EMBED_LN_QUANT launch_bert_i8_embed_ln_quant.  ids, positions [m]; in: word [vocab, hidden], pos [max_pos, hidden], type0 [hidden],
 *                  ln_w, ln_b; out_f32 = x [m, hidden], out_codes [m, hidden], out_scales [m]
 *   ADD_LN_QUANT   launch_bert_i8_add_ln_quant.  in: x [m, hidden] (updated in place on the device), delta [m, hidden], ln_w, ln_b;
 *                  out_f32 = x.  form 0: out_codes, out_scales as above.  form 1 passes q = NULL as the last layer does: out_codes and
 *                  out_scales are not written (they may be NULL); the lab still holds guard-filled code and scale buffers and returns
 *                  FSGPU_ERR_DEVICE if the kernel touched them */
#define FSGPU_LAB_BERT_I8_QUANT_ROWS 0
#define FSGPU_LAB_BERT_I8_PACK_W 1
#define FSGPU_LAB_BERT_I8_GEMM 2
#define FSGPU_LAB_BERT_I8_EMBED_LN_QUANT 3
#define FSGPU_LAB_BERT_I8_ADD_LN_QUANT 4
typedef struct fsgpu_lab_bert_int8_stage_args {
    uint32_t stage, form, epilogue;
    uint32_t m, n, k, hidden, vocab, max_pos;
    float eps;
    const int32_t *ids, *positions;
    const int8_t *codes;
    const float *in[5];
    float *out_f32;
    int8_t *out_codes;
    float *out_scales;
} fsgpu_lab_bert_int8_stage_args;
fsgpu_status fsgpu_lab_bert_int8_stage(int32_t device, const fsgpu_lab_bert_int8_stage_args *args);
/* ONE stage of the two short-text forwards on host arrays, through the launcher the embedder calls and with the argument block filled
 * as NativeEmbedder::forward_query / embed_docs fill it: for kernel-level tests against tests/encoder_short_ref.py.  MiniLM-L6 shape
 * only (hidden 384, inter 1536, heads 12; anything else is FSGPU_ERR_INVALID_CONFIG, nothing launched; arguments are checked before a
 * device is looked for).  f16 operands are rounded on the device, f16 outputs come back widened, every output lies between guard bands
 * as for fsgpu_lab_bert_stage.
 * Query stages (bert_query_kernels.hip): m tokens in 1..32, offsets [n_docs + 1] from 0 to m (empty texts allowed).  Workspaces are laid
 * out as the product's: X [32][384], slabs [slab][32][384], ctx / inter [tokens][n]; rows m..31 of every INPUT workspace hold NaN; an
 * output is its m rows; the four-slab output's whole 4 x 32-row region is prefilled with the guard byte and rows m..31 of each slab must
 * keep it (else FSGPU_ERR_DEVICE, "guard band").
 *   Q_ATTN  launch_bert_q_qkv_attn.  form 0 (embedding prologue): ids, positions [m]; in: word [vocab, 384], pos [max_pos, 384],
 *           type0 [384], ln_w, ln_b, wqkv [1152, 384], bqkv [1152].  form 1 (pending add + LayerNorm of four slabs): in: x_in [m, 384],
 *           parts [4, m, 384], prev_bias, ln_w, ln_b, wqkv, bqkv.  out0 = ctx [m, 384] (f16), out1 = x_out [m, 384] (f32)
 *   Q_GEMM  launch_bert_q_gemm, form = its mode.  0: in: a [m, 384], w [384, 384]; out0 = one slab [m, 384] (f32, no bias).
 *           1: in: x_in, slab [m, 384], prev_bias, ln_w, ln_b, w [1536, 384], bias [1536]; out0 = GELU tile [m, 1536] (f16), out1 = x_out.
 *           2: in: a [m, 1536], w [384, 1536]; out0 = the four slabs [4, m, 384]
 *   Q_POOL  launch_bert_q_pool.  in: x_in, parts [4, m, 384], prev_bias, ln_w, ln_b; out0 = [n_docs, 384]
 * DOCS (bert_docs_w.hip): launch_bert_docs_w over `layers` in 1..6 layers; ids [m], offsets of texts of at most 32 tokens each (m >= 1),
 * packed into row blocks by the embedder's own bert_docs_pack.  in: word, pos, type0, emb_ln_w, emb_ln_b; layer_in [layers][12]: wqkv
 * [1152, 384], bqkv, wao [384, 384], bao, ln1_w, ln1_b, wi [1536, 384], bi, wo [384, 1536], bo, ln2_w, ln2_b (matrices rounded to f16
 * and re-laid in fragment order as at model load).  out0 = pooled [n_docs, 384] */
#define FSGPU_LAB_BERT_Q_ATTN 0
#define FSGPU_LAB_BERT_Q_GEMM 1
#define FSGPU_LAB_BERT_Q_POOL 2
#define FSGPU_LAB_BERT_DOCS 3
typedef struct fsgpu_lab_bert_short_args {
    uint32_t stage, form;
    uint32_t m, n_docs, hidden, inter, heads, layers, vocab, max_pos;
    float eps, scale;
    const uint32_t *offsets;
    const int32_t *ids, *positions;
    const float *in[8];
    const float *const *layer_in;
    float *out0, *out1;
} fsgpu_lab_bert_short_args;
fsgpu_status fsgpu_lab_bert_short_stage(int32_t device, const fsgpu_lab_bert_short_args *args);
/* ONE stage of the batched scan on host arrays, through the launcher the product calls (launch_scan_mfma, launch_scan_wide,
 * launch_prepare_queries, launch_prepare_queries_i8) with an MfmaScanArgs filled from this struct: for kernel-level tests against
 * tests/scan_stage_ref.py.  One launch on the default stream, fresh device buffers, no kernel of its own.
 *   kernel  LDS (queries in LDS, mfma_scan.hip): variant = shape, stage 0 dense sample / 1 thresholded sample / 2 main pass (every
 *           64-row group outside the sample {j group_stride : j < group_count}; group_stride >= 1).
 *           REG (queries in registers, mfma_wide.hip): variant = query tiles per wave, stage 1 thresholded sample / 2 main pass (every
 *           row) / 3 group maxima (int8 rows: cand is [nq_pad][grid][4], no tau, no spill).
 *           PREPARE: queries_f32 [nq, dim] -> prepared [nq_pad, dim] (f16 bits for elem_bytes 2 with max_norm_bits, int8 levels for
 *           elem_bytes 1 with bits 8 or 4) and delta [nq_pad]; nothing else is read.
 *   A launch answers `groups` (0 means 1) query groups of the kernel's size (16 x the shape's query tiles; 128 x variant): nq_pad must be
 *   groups x that size.  A sample's groups must all begin below nrows.  slab: nrows rows of row_stride (0: dim x elem_bytes) bytes; live /
 *   allow: ceil(nrows / 64) words or NULL; queries: nq_pad x dim elements as the kernel reads them; tau [nq_pad].
 *   Outputs (those the stage writes must not be NULL): cand [nq_pad][grid][slots], cand_count [nq_pad][grid] (REG, want_counts = 1: the
 *   lists are then NOT padded), spill [nq_pad][spill_cap], spill_count [nq_pad x 16] (the product's counter stride), overflow [nq_pad],
 *   dense [nq_pad][group_count x 64].  List, spill and dense areas are prefilled with bytes 0xCD, the counters and flags with zero.
 * Arguments are checked before a device is looked for (fsgpu_lab_scan_stage_check does only that: FSGPU_OK = it would be launched); what
 * the launchers' own predicates refuse, and a shape this build does not contain, is FSGPU_ERR_INVALID_CONFIG with nothing launched.
 * Every output lies between guard bands of a fixed pattern (FSGPU_ERR_DEVICE, "guard band", if one is touched); behind the slab's last
 * row lie guard rows of NaN (f16) or 0x7f (int8), so a read past nrows that reaches a score shows in the answers.  The grid need not
 * fit the chip: the kernels' blocks are independent. */
#define FSGPU_LAB_SCAN_LDS 0
#define FSGPU_LAB_SCAN_REG 1
#define FSGPU_LAB_SCAN_PREPARE 2
typedef struct fsgpu_lab_scan_stage_args {
    uint32_t kernel, variant, stage, elem_bytes, dim, nrows, row_stride, row_base;
    uint32_t grid, groups, side_by_side, reverse, group_stride, group_count, slots, spill_cap, nq_pad, want_counts;
    uint32_t nq, max_norm_bits, bits, reserved;
    const void *slab;
    const uint64_t *live, *allow;
    const void *queries;
    const float *tau;
    const float *queries_f32;
    uint64_t *cand;
    uint32_t *cand_count;
    uint64_t *spill;
    uint32_t *spill_count, *overflow;
    uint64_t *dense;
    void *prepared;
    float *delta;
} fsgpu_lab_scan_stage_args;
fsgpu_status fsgpu_lab_scan_stage_check(const fsgpu_lab_scan_stage_args *args);
fsgpu_status fsgpu_lab_scan_stage(int32_t device, const fsgpu_lab_scan_stage_args *args);
/* The 128-query shape of the LDS-query kernel the batched planner runs when FSGPU_MFMA_SHAPE (elem_bytes 2) or FSGPU_MFMA_SHAPE_I8
 * (elem_bytes 1) asks for `requested` (0: nothing asked): a shape this build does not contain is never chosen. */
int32_t fsgpu_lab_scan_planner_shape(int32_t requested, int32_t elem_bytes);
/* ONE selection of the batched search on host arrays, through the launcher the product calls (launch_select, launch_select_groups,
 * launch_list_cut, launch_two_pass_merge) with a SelectArgs / GroupSelectArgs filled field for field from this struct: for kernel-level
 * tests against tests/selection_ref.py.  Default stream, fresh device buffers, no kernel of its own.  nq blocks are launched.
 *   SELECT        lists: nq x q_stride entries (q_stride >= (nlists - 1) l_stride + list_len); list_counts [nq][nlists] or NULL;
 *                 extra [nq][extra_len]; spill [nq][spill_cap] with spill_count [nq x 16] (the product's counter stride; in: the counts, out:
 *                 what the launch left).  reset_spill = 1: SelectArgs::spill_reset IS spill_count, as the product always passes it.
 *                 slab != NULL makes it a finish step (rows of row_stride bytes, 0 = dense; f32 rows with slab_f32); queries holds
 *                 valid_queries rows (nq when that is 0) of query_stride (0 = dim) floats and is followed on the device by NaN rows, so a
 *                 padding block that reads its query shows.  pool_flag [nq] (in: initial contents, out: final) or NULL.
 *                 big_pool 0: one launch (pool_flag as given).  1: the product's two launches over the same lists, the first with
 *                 big_pool = 0 (it fills pool_flag), the second with big_pool = 1.  2: the second-chance launch alone, on the flags given.
 *   SELECT_GROUPS lists = groups [nq][nentries]; delta, anchor_unit, tau_out, overflow, spill_count / reset_spill, slab (dense rows),
 *                 live / allow (ceil(nrows / 64) words or NULL), queries, dim, nrows, row_base, query_stride, hreduce, valid_queries,
 *                 slab_f32, rank_only as in GroupSelectArgs.
 *   LIST_CUT      lists [nlists][list_len]; tau_out[0] receives the cut.
 *   TWO_PASS_MERGE lists = the pass-1 entries, exact_lists = the exact ones: nshards x shard_pitch entries each (shard_pitch >= nq x cc);
 *                 k, out_stride, out_rows, out_scores, out_counts.
 * Output areas a launch may write (those given non-NULL) are prefilled with bytes 0xCD, `overflow` with zero, and lie between guard bands
 * (FSGPU_ERR_DEVICE, "guard band", if one is touched); the slab is followed by guard rows of NaN.  Arguments are checked before a device is
 * looked for (fsgpu_lab_select_check does only that: FSGPU_OK = it would be launched); what the launchers' own predicates refuse
 * (select_args_ok, select_groups_args_ok, list_cut_args_ok, two_pass_merge_args_ok of kernels.hpp) is FSGPU_ERR_INVALID_CONFIG with
 * nothing launched. */
#define FSGPU_LAB_SELECT 0
#define FSGPU_LAB_SELECT_GROUPS 1
#define FSGPU_LAB_LIST_CUT 2
#define FSGPU_LAB_TWO_PASS_MERGE 3
typedef struct fsgpu_lab_select_args {
    uint32_t kernel, nq, valid_queries, k;
    uint64_t q_stride, shard_pitch;
    uint32_t l_stride, nlists, list_len, extra_len, spill_cap, reset_spill, take_topk, heur_rank, big_pool;
    uint32_t dim, nrows, row_base, row_stride, query_stride;
    int32_t hreduce;
    uint32_t k_out, out_stride, cand_out_stride, slab_f32, nentries, rank_only, nshards, cc;
    const uint64_t *lists;
    const uint32_t *list_counts;
    const uint64_t *extra, *spill, *exact_lists;
    const float *delta, *anchor_unit, *tau_floor_in;
    const void *slab;
    const uint64_t *live, *allow;
    const float *queries;
    uint32_t *spill_count, *pool_flag;
    float *tau_out, *tau_floor_out;
    uint64_t *pool_out;
    uint32_t *cand_counts, *overflow;
    uint32_t *out_rows;
    float *out_scores;
    uint64_t *out_packed;
    uint32_t *out_counts;
    uint64_t *cand_approx_out, *cand_exact_out;
} fsgpu_lab_select_args;
fsgpu_status fsgpu_lab_select_check(const fsgpu_lab_select_args *args);
fsgpu_status fsgpu_lab_select(int32_t device, const fsgpu_lab_select_args *args);
/* ONE launch of the per-query search path on host arrays, through the launcher the product calls (launch_scan_topk,
 * launch_scan_topk_host_query, launch_scan_mq, launch_scan_i8, launch_scan_4bit, launch_scan_topk_f32, launch_merge_topk) with a
 * ScanArgs / MergeArgs filled field for field from this struct and an EXPLICIT grid: for kernel-level tests against
 * tests/lone_scan_ref.py.  Default stream, fresh device buffers, no kernel of its own, one synchronisation.
 *   scans  nq = queries per pass (F16 1 / 2 / 4; F16_HOST_QUERY, I8, I4 1; F16_MQ 4 / 8; F32 1 / 2 / 4), tier = 64 / 256 (the kernels'
 *          KCAP), 1 <= k <= tier, 1 <= grid <= 4096, nrows >= 1.  slab: nrows rows of row_stride bytes (0 = dense: dim x 2 for f16, dim x 4
 *          for F32, dim for I8, dim / 2 packed nibbles, low nibble = even dimension, for I4; a strided view — a multiple of 16 bytes that
 *          holds a row — only where the kernel reads ScanArgs::row_stride: F16, F16_HOST_QUERY, F32).  queries: nq x dim f32 (F16_HOST_QUERY:
 *          read from this host array at launch), or the quantised query as the kernel reads it (I8: dim int8, I4: dim / 2 bytes).
 *          live / allow: bitmap_words words each (>= ceil(nrows / 64)) or NULL.  force_runtime_dim / plain_loads: launch_scan_topk's (F16
 *          only).  partial [nq][grid][k] receives one best-first list per (query, block), kEmpty padded.
 *   MERGE  lists: nq x q_stride entries (q_stride >= (nlists - 1) l_stride + list_len, l_stride >= list_len >= 1, nlists >= 1),
 *          1 <= k <= 256, out_stride >= k, lists_sorted 0 / 1; any subset of out_rows / out_scores / out_packed [nq][out_stride] and
 *          out_counts [nq].
 * Output areas are prefilled with bytes 0xCD and lie between guard bands (FSGPU_ERR_DEVICE, "guard band", if one is touched); the slab is
 * followed by guard rows of NaN (f16, f32) or 0x7f (int8, 4-bit).  Arguments are checked before a device is looked for
 * (fsgpu_lab_lone_stage_check does only that: FSGPU_OK = it would be launched); what the launchers or their *_supported predicates
 * refuse, and what the kernels cannot hold, is FSGPU_ERR_INVALID_CONFIG with nothing launched. */
#define FSGPU_LAB_LONE_F16 0
#define FSGPU_LAB_LONE_F16_HOST_QUERY 1
#define FSGPU_LAB_LONE_F16_MQ 2
#define FSGPU_LAB_LONE_I8 3
#define FSGPU_LAB_LONE_I4 4
#define FSGPU_LAB_LONE_F32 5
#define FSGPU_LAB_LONE_MERGE 6
typedef struct fsgpu_lab_lone_stage_args {
    uint32_t kind, nq, tier, dim, nrows, row_stride, row_base, k, grid, force_runtime_dim, plain_loads;
    int32_t hreduce;
    uint32_t bitmap_words, nlists, list_len, l_stride, out_stride, lists_sorted;
    uint64_t q_stride;
    const void *slab;
    const uint64_t *live, *allow;
    const void *queries;
    uint64_t *partial;
    const uint64_t *lists;
    uint32_t *out_rows;
    float *out_scores;
    uint64_t *out_packed;
    uint32_t *out_counts;
} fsgpu_lab_lone_stage_args;
fsgpu_status fsgpu_lab_lone_stage_check(const fsgpu_lab_lone_stage_args *args);
fsgpu_status fsgpu_lab_lone_stage(int32_t device, const fsgpu_lab_lone_stage_args *args);
/* fsgpu_index_compute_query_hubness that also returns what it selected: out_topk[record_count, min(kq, nq)] holds every row's
 * selected similarities, greatest first under total_cmp (for tests of the selection itself; meant for small indexes). */
fsgpu_status fsgpu_lab_index_query_hubness_topk(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                                float *out, float *out_topk);
/* What the batched search reported to the last fsgpu_index_build_knn_graph on this handle, summed over its steps: out[0] steps,
 * out[1] live sources searched, out[2] queries answered by the exact kernels (fallbacks), out[3] queries answered in a step's end
 * half (fallbacks + queries the int8 filter handed to the f16 filter). */
fsgpu_status fsgpu_lab_index_knn_build_stats(fsgpu_index *idx, uint64_t *out4);
/* ---- compaction (fsgpu_index_compact / _vacuum) ---- */
/* Destination rows one launch of the segmented-copy kernel covers (0 = the default, 2^20): lets a test cross launch boundaries with a
 * few thousand rows. */
fsgpu_status fsgpu_lab_index_set_compact_launch_rows(fsgpu_index *idx, uint32_t rows);
/* The kernel's stores with (1) / without (0, default) the non-temporal hint: the A/B of DESIGN 3.12. */
fsgpu_status fsgpu_lab_index_set_compact_nt_stores(fsgpu_index *idx, int32_t enabled);
/* What the last rewrite cost: out_ms5 = plan (merge, runs, upload, WAL encode), kernel launches until done, table rebuild, file,
 * rebuild of derived copies; out_counts3 = runs, launches, destination bytes. */
fsgpu_status fsgpu_lab_index_last_rewrite(fsgpu_index *idx, double *out_ms5, uint64_t *out_counts3);
/* Gives an index made from a bare slab (fsgpu_index_create / _create_device) a doc-id table: the ids "doc-000000000", ... assigned so
 * that the rows as they stand are in (hash, doc id) order.  For measurements of the write path on a generated corpus. */
fsgpu_status fsgpu_lab_index_attach_synthetic_doc_ids(fsgpu_index *idx);
/* The arithmetic of wal_topk_kernel (fsgpu_search_hits_batched) on its own: out[q * W + w] = the kernel's dot_product_f32_f32 of
 * resident WAL entry w with host query q, W = fsgpu_index_wal_record_count, non-finite scores included.  Builds the device
 * mirror of the WAL if need be. */
fsgpu_status fsgpu_lab_index_wal_scores(fsgpu_index *idx, const float *queries, uint32_t nq, float *out);
/* The yardstick of the copy kernel: `reps` hipMemcpyDtoD of `bytes` between two fresh buffers, each timed by events (ms). */
fsgpu_status fsgpu_lab_device_copy_ms(int32_t device, uint64_t bytes, uint32_t reps, double *out_ms);
/* fsgpu_hash_embed with the device's own time of its three stages, between events on the embedder's stream (ms):
 * out_stage_ms[3] = {texts and offsets to the device, the kernel, vectors back to `out`}. */
fsgpu_status fsgpu_lab_hash_embed_stage_ms(fsgpu_hash *h, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n, float *out,
                                           float *out_stage_ms);
/* fsgpu_wordpiece_encode with the device's own time of its stages, between events on the tokenizer's stream (ms):
 * out_stage_ms[3] = {texts, offsets and piece regions to the device; the tokenize and offsets kernels, the host's read of the
 * total, the assemble kernel; ids and offsets back to the host}. */
fsgpu_status fsgpu_lab_wordpiece_encode_stage_ms(fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n,
                                                 int32_t add_special_tokens, uint32_t max_length, uint32_t *out_ids,
                                                 uint64_t ids_capacity, uint32_t *out_offsets, float *out_stage_ms);
/* ONE launch of knn_update_join_kernel (fsgpu_index_update_knn_graph) through the guard-band harness: slab [nrows, dim]
 * f16 (or f32 with slab_f32), dense rows; classes [nrows] (0 dead, 1 added, 2 kept-clean, 3 kept-dirty); work [nrows, m] IN AND OUT,
 * a row's list as packed entries (score bits << 32 | local row), best first, ~0 past its end; added [n_added, dim] the added rows
 * widened to f32 and added_rows [n_added] their local rows, 1 <= n_added <= 1,024.  Only kept-clean rows' lists may change.  The
 * slab is followed by NaN guard rows and the working table sits between guard bands: a touched band is FSGPU_ERR_DEVICE. */
fsgpu_status fsgpu_lab_knn_update_join(int32_t device, const void *slab, uint32_t slab_f32, uint32_t nrows, uint32_t dim, int32_t hreduce,
                                       uint32_t m, const uint8_t *classes, uint64_t *work, const float *added, const uint32_t *added_rows,
                                       uint32_t n_added);
/* ---- the IVF index's int8 list filter (fsgpu_ivf_set_list_filter) ---- */
/* One search of a handle with the filter on, its filter stage through the guard-band harness: the scores, the per-slot results and
 * the candidates are written by the kernels into buffers that sit between guard bands (a touched band, or a padding entry of the
 * scores that is not the dead-row sentinel, is FSGPU_ERR_DEVICE).  The call must fit the scratch at once and k <= 64.
 *   out_ordered      [lists' rows, dimension] int8: the LOGICAL ordered copy, ordered[p] = filter_i8[list_rows[p]] (nullable)
 *   out_delta        [nq] the bound of each query against the handle's statistics (< 0: uncertified)
 *   out_ran          0: no query was certified (or no slot exists) and the filter stage did not run; everything below is then unwritten
 *   out_nslots       the slots: (list, query) pairs of the non-empty probed lists, by list, then by query
 *   out_slot_query, out_slot_list   [slots]
 *   out_slot_offset  [slots + 1]: slot s owns out_scores[out_slot_offset[s] .. out_slot_offset[s + 1]), one entry per row of its list in
 *                    list order: the int32 dot of the query's codes with the row's, INT32_MIN for a dead row
 *   out_t, out_m, out_count, out_flag   [slots]: the k-th largest score (INT32_MIN when no more than k rows are live), ceil(2 delta),
 *                    the candidates (never clipped), 1 = overflowed | 2 = uncertified (t, m, count then 0 / INT32_MIN)
 *   out_cand         [slots, 128]: the first min(count, 128) candidates, local rows ascending; the rest keeps the byte 0xA5
 * slots_cap / scores_cap: what the caller's arrays hold (nq * nprobe slots and fsgpu_ivf_stats.rows_scored entries always do). */
typedef struct fsgpu_lab_ivf_filter_stage_args {
    const float *queries;   /* HOST [nq, query_len] */
    uint32_t nq, query_len, k, nprobe;
    uint32_t slots_cap, reserved0;
    uint64_t scores_cap;
    int8_t *out_ordered;
    float *out_delta;
    uint32_t *out_ran, *out_nslots, *out_slot_query, *out_slot_list;
    uint64_t *out_slot_offset;
    int32_t *out_scores, *out_t;
    int64_t *out_m;
    uint32_t *out_count, *out_flag, *out_cand;
} fsgpu_lab_ivf_filter_stage_args;
fsgpu_status fsgpu_lab_ivf_filter_stage(fsgpu_ivf *ivf, const fsgpu_lab_ivf_filter_stage_args *args);
/* The scores the filter keeps resident at once (0: the default, 2^26): lets a test cross the range split, and put a tile above the
 * scratch, with lists of a few hundred rows. */
fsgpu_status fsgpu_lab_ivf_filter_set_scratch(fsgpu_ivf *ivf, uint64_t entries);
/* The filter's two host plans (ivf_filter_plan.hpp) on their own; no device is needed.  offsets [nlist + 1] the lists, members
 * [nlist] the queries that probe each list.
 * score plan: out_tiles [tiles_cap][8] = ordered_row0, list_pos0, scratch0, len, slot0, nmem, item0, above-the-scratch;
 *             out_ranges [ranges_cap][7] = tile_first, ntiles, item_first, nitems, slot_first, nslots, entries.
 * scan plan:  counts, flags [slots] as the selection reports them; out_groups [groups_cap][6] = rows_off, from_cand, n, q0, nq, nblocks.
 * A capacity too small for the result is FSGPU_ERR_INVALID_CONFIG. */
fsgpu_status fsgpu_lab_ivf_filter_score_plan(uint32_t nlist, const uint64_t *offsets, const uint32_t *members, uint64_t scratch_cap,
                                             uint32_t tiles_cap, uint64_t *out_tiles, uint32_t *out_ntiles, uint32_t ranges_cap,
                                             uint64_t *out_ranges, uint32_t *out_nranges, uint32_t *out_slots);
fsgpu_status fsgpu_lab_ivf_filter_scan_plan(uint32_t nlist, const uint64_t *offsets, const uint32_t *members, const uint32_t *counts,
                                            const uint32_t *flags, uint32_t k, uint32_t num_cus, uint32_t groups_cap, uint64_t *out_groups,
                                            uint32_t *out_ngroups, uint32_t *out_grid_x, uint64_t *out_rows_rescored);
/* Selects the scan kernel variant (0 = default) — used by bench A/B runs only. */
fsgpu_status fsgpu_index_set_variant(fsgpu_index *idx, int32_t variant);

#ifdef __cplusplus
}
#endif
#endif /* FSGPU_LAB_H */

/*
 * fsgpu.h — C ABI of libfsgpu.so, the MI355X (gfx950) semantic tier for frankensearch.
 *
 * The reference has no FFI for this path: its seams are Rust traits and one concrete method
 * set.  Each entry point below names the reference interface it replaces
 * (file:line relative to the reference repo) so a ~100-line Rust shim can bind it
 * (see INTEGRATION.md for that shim).
 *
 * Conventions
 *   - every function returns an fsgpu_status (0 = OK); no exception crosses the boundary;
 *   - fsgpu_last_error() returns the calling thread's last failure detail (UTF-8);
 *   - all pointers are caller-owned unless stated; "_dev" pointers are HIP device pointers;
 *   - handles may be used from many host threads.  fsgpu_search_topk calls (row-level searches, filtered or not) from
 *     different threads run side by side on up to four lanes of an index (own HIP stream and workspaces each) — the
 *     reference's scan is `&self` and lock-free (search.rs:192); every other call on a handle serialises internally, and
 *     calls that change an index (tombstones, WAL, live bitmap) wait for the searches in flight;
 *   - row ids are GLOBAL physical row ids (row_base + local row), u32 like VectorHit.index
 *     (crates/frankensearch-core/src/types.rs:88-95);
 *   - result order is the reference's: score descending with NaN ranked as -inf, f32 total
 *     order (-0.0 < +0.0), ties by ascending row (crates/frankensearch-index/src/search.rs:1655-1686);
 *   - scores are computed in the reference's exact accumulation order (simd.rs:398-446), so they
 *     are bit-identical to the CPU path's scores for a given FSGPU_HREDUCE_* mode.
 */
#ifndef FSGPU_H
#define FSGPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t fsgpu_status;

/* Status codes <-> SearchError variants (crates/frankensearch-core/src/error.rs:57-176). */
#define FSGPU_OK 0
#define FSGPU_ERR_DIMENSION_MISMATCH 1     /* SearchError::DimensionMismatch{expected,found} */
#define FSGPU_ERR_INVALID_CONFIG 2         /* SearchError::InvalidConfig{field,value,reason} */
#define FSGPU_ERR_INDEX_CORRUPTED 3        /* SearchError::IndexCorrupted{path,detail} */
#define FSGPU_ERR_INDEX_VERSION_MISMATCH 4 /* SearchError::IndexVersionMismatch{expected,found} */
#define FSGPU_ERR_IO 5                     /* SearchError::Io */
#define FSGPU_ERR_DEVICE 6                 /* HIP runtime failure (no reference analogue) */
#define FSGPU_ERR_NO_DEVICE 7              /* no gfx950 device visible */
#define FSGPU_ERR_NULL_ARGUMENT 8
#define FSGPU_ERR_EMBEDDING_FAILED 9       /* SearchError::EmbeddingFailed */
#define FSGPU_ERR_MODEL_LOAD_FAILED 10     /* SearchError::ModelLoadFailed{path,source} */

/* ZeroSignalReason of search_top_k_classified (search.rs:227-261). */
#define FSGPU_ZERO_SIGNAL_NONE 0
#define FSGPU_ZERO_SIGNAL_CALLER_REQUESTED_ZERO_K 1
#define FSGPU_ZERO_SIGNAL_ZERO_NORM_QUERY 2
/* empty_result_reason (crates/frankensearch-core/src/config.rs:696-740) for a well-formed search that came back empty.  The
 * classified entry point takes no filter, so FILTER_ELIMINATED_ALL and NO_USABLE_VECTORS (an exact scan returns every live
 * row, whatever its score) are listed for callers that classify filtered searches themselves. */
#define FSGPU_ZERO_SIGNAL_FILTER_ELIMINATED_ALL 3
#define FSGPU_ZERO_SIGNAL_NEWLY_CREATED_EMPTY 4      /* no main records, no WAL entries */
#define FSGPU_ZERO_SIGNAL_ALL_TOMBSTONED 5           /* every main record tombstoned, no WAL entry */
#define FSGPU_ZERO_SIGNAL_WAL_ONLY_NO_LIVE_RECORDS 6 /* no live main record; the WAL entries produced no usable hit */
#define FSGPU_ZERO_SIGNAL_NO_USABLE_VECTORS 7

/* Order of the final 8-lane horizontal add (`wide::f32x8::reduce_add`, simd.rs:439,563).
 * SSE2 is the reference's default build (no +avx2 in .cargo/config.toml). */
#define FSGPU_HREDUCE_SSE2 0 /* ((v0+v2)+(v1+v3)) + ((v4+v6)+(v5+v7)) */
#define FSGPU_HREDUCE_AVX 1  /* ((v0+v4)+(v2+v6)) + ((v1+v5)+(v3+v7)) */
#define FSGPU_HREDUCE_SEQ 2  /* (((v0+v1)+v2)+v3) + (((v4+v5)+v6)+v7): f32x8 as a.reduce_add() + b.reduce_add() over a
                              * left-to-right f32x4 sum (the fallback shape `wide` has shipped); INTEGRATION.md shows how a
                              * maintainer finds out which of the three the Rust build uses */

typedef struct fsgpu_index fsgpu_index;     /* device-resident VectorIndex (lib.rs:819) */
typedef struct fsgpu_m2v fsgpu_m2v;         /* Model2VecEmbedder (embed/src/model2vec_embedder.rs:55) */
typedef struct fsgpu_hash fsgpu_hash;       /* HashEmbedder (embed/src/hash_embedder.rs:201) */
typedef struct fsgpu_wordpiece fsgpu_wordpiece; /* the BERT WordPiece tokenizer (third-party `tokenizers` in the reference) */
typedef struct fsgpu_bert fsgpu_bert;       /* NativeEmbedder (rerank/src/native_embedder.rs:40-50) */
typedef struct fsgpu_reranker fsgpu_reranker; /* NativeReranker, the cross-encoder (rerank/src/native.rs:1240) */

/* BERT shape (all-MiniLM-L6-v2: vocab 30522, hidden 384, layers 6, heads 12, inter 1536, max_pos 512,
 * ln_eps 1e-12; crates/frankensearch-rerank/src/native.rs:36-45).  heads*32 must equal hidden. */
typedef struct fsgpu_bert_config {
    uint32_t vocab, hidden, layers, heads, inter, max_pos;
    float ln_eps;
} fsgpu_bert_config;
/* One encoder layer in HuggingFace tensor layout ([out, in] row-major f32), the keys parse_weights reads
 * (native.rs:1359-1602): attention.self.{query,key,value}, attention.output.{dense,LayerNorm},
 * intermediate.dense, output.{dense,LayerNorm}. */
typedef struct fsgpu_bert_layer_weights {
    const float *q_w, *q_b, *k_w, *k_b, *v_w, *v_b;
    const float *ao_w, *ao_b, *ln1_w, *ln1_b;
    const float *i_w, *i_b, *o_w, *o_b, *ln2_w, *ln2_b;
} fsgpu_bert_layer_weights;
typedef struct fsgpu_bert_weights {
    const float *word_emb, *pos_emb, *type_emb, *emb_ln_w, *emb_ln_b;
    const fsgpu_bert_layer_weights *layers; /* [config.layers] */
} fsgpu_bert_weights;

/* ---- library ---- */
const char *fsgpu_version(void);
int32_t fsgpu_device_count(void);
const char *fsgpu_last_error(void);

/* ---- index lifecycle ---- */
/* Replaces VectorIndex::open + the mmap of the slab (lib.rs:1747-1816): copies `nrows` x `dim`
 * little-endian f16 rows from host memory to device `device`.  live_bitmap (bit r = row r is live,
 * i.e. RECORD_FLAG_TOMBSTONE clear, lib.rs:171-173) may be NULL = all live.  row_base is added to
 * every reported row id (shard offset). */
fsgpu_status fsgpu_index_create(int32_t device, uint32_t dim, uint64_t nrows, const void *slab_f16_le,
                                const uint64_t *live_bitmap, uint64_t row_base, fsgpu_index **out);
/* Zero-copy variant: adopts (does not free) a device-resident slab / bitmap. */
fsgpu_status fsgpu_index_create_device(int32_t device, uint32_t dim, uint64_t nrows, const void *slab_f16_dev,
                                       const uint64_t *live_bitmap_dev, uint64_t row_base, fsgpu_index **out);
/* The same two doors for a Quantization::F32 slab (lib.rs:203-208; rows are raw little-endian f32, scored in
 * dot_product_f32_bytes_f32's order, simd.rs:581-702): an f32 matrix the caller holds becomes an index without a detour through an
 * FSVI file or the index builder.  Everything an FSVI-opened F32 index does, these do. */
fsgpu_status fsgpu_index_create_f32(int32_t device, uint32_t dim, uint64_t nrows, const void *slab_f32_le,
                                    const uint64_t *live_bitmap, uint64_t row_base, fsgpu_index **out);
fsgpu_status fsgpu_index_create_f32_device(int32_t device, uint32_t dim, uint64_t nrows, const void *slab_f32_dev,
                                           const uint64_t *live_bitmap_dev, uint64_t row_base, fsgpu_index **out);
/* VectorIndex::open for an FSVI v1 / F16 file (lib.rs:4049-4144 header+CRC, :3510-3537 record table):
 * uploads the slab, builds the live bitmap from record flags, keeps the doc-id table on the host. */
fsgpu_status fsgpu_index_open_fsvi(const char *path, int32_t device, fsgpu_index **out);
void fsgpu_index_destroy(fsgpu_index *idx);

uint64_t fsgpu_index_record_count(const fsgpu_index *idx); /* VectorIndex::record_count */
uint32_t fsgpu_index_dimension(const fsgpu_index *idx);    /* VectorIndex::dimension */
fsgpu_status fsgpu_index_set_hreduce(fsgpu_index *idx, int32_t mode);
/* doc id of a global row (FSVI-opened indexes only; pointer valid until destroy; not NUL-terminated). */
fsgpu_status fsgpu_index_doc_id(const fsgpu_index *idx, uint32_t row, const char **ptr, uint32_t *len);
/* VectorIndex::soft_delete = soft_delete_batch(&[id]) > 0 (lib.rs:2303-2397): clears the live bit of every main row with
 * that doc id AND drops its resident WAL entries; *deleted = 1 if anything went live -> deleted. */
fsgpu_status fsgpu_index_soft_delete(fsgpu_index *idx, const char *doc_id, uint32_t doc_id_len, int32_t *deleted);
/* SearchFilter::candidate_hashes -> rows (gather_positions_for_hashes / hash_range, search.rs:1146-1198): sets, in
 * allow_bitmap_out (ceil(record_count / 64) words, cleared first), the bit of every main row whose record hash
 * (FNV-1a 64 of the doc id, lib.rs:6120-6127) is one of `hashes` — a binary search per hash in the (hash, doc_id)-
 * sorted record table.  The bitmap is what fsgpu_search_topk takes as its filter (tombstoned rows are masked there).
 * FSVI-opened indexes only.  *rows_matched (may be NULL) = bits set. */
fsgpu_status fsgpu_index_allow_bitmap_for_hashes(const fsgpu_index *idx, const uint64_t *hashes, uint32_t n,
                                                 uint64_t *allow_bitmap_out, uint64_t *rows_matched);
/* VectorIndex::append (lib.rs:2532-2720): a resident WAL entry (f32 vector, immediately searchable through
 * fsgpu_search_hits with the reference's scan_wal / shadowing rules, search.rs:1449-1475,1503-1558); supersedes a
 * resident entry with the same doc id and tombstones the first live main row with that doc id.  The WAL *file*
 * (durability) stays with the caller.  FSVI-opened indexes only. */
fsgpu_status fsgpu_index_wal_append(fsgpu_index *idx, const char *doc_id, uint32_t doc_id_len, const float *vector,
                                    uint32_t vector_len);
uint64_t fsgpu_index_wal_record_count(const fsgpu_index *idx); /* VectorIndex::wal_record_count */
/* VectorIndex::append_batch (lib.rs:2546-2720): n entries, vectors [n, vector_len] row-major.  EVERY entry is validated before
 * anything changes (dimension, finite values, usable norm, doc id <= u16 bytes: one bad entry and the index is as it was); a doc id
 * repeated inside the batch keeps its last vector (lib.rs:2604-2615); resident copies are superseded; the first live main row of each
 * doc id is tombstoned; the live bitmap goes up ONCE.  fsgpu_index_wal_append is a batch of one. */
fsgpu_status fsgpu_index_wal_append_batch(fsgpu_index *idx, uint32_t n, const char *const *doc_ids, const uint32_t *doc_id_lens,
                                          const float *vectors, uint32_t vector_len);

/* ---- compaction and vacuum: the WAL and the tombstones folded into the slab, on the device ----
 * Both calls replace the index's slab by a new one that holds the surviving rows only (an HBM-to-HBM segmented copy into a fresh
 * allocation: transiently both slabs are resident), rebuild the record tables on the host and clear every record flag.
 * path = NULL: device only.  path != NULL: the new FSVI v1 image is ALSO written — rewrite_index's layout (lib.rs:2871-3094): header
 * with CRC32, 16-byte records, string table, padding to 64, slab — under a temporary name beside the target and renamed over it.  The
 * WAL sidecar file stays the caller's business, as for fsgpu_index_wal_append.
 * Failure: the new slab is allocated before anything is touched; if that, the copy or the file write fails, the error is returned and
 * the index is exactly as it was (slab, bitmap, tables, WAL, generations).
 * Quiescence: NO search may be in flight on the handle.  The calls take the index's lock and every lane's, and are refused with
 * FSGPU_ERR_INVALID_CONFIG while a ticket of fsgpu_search_topk_batched_device_begin is outstanding.  Row-sharded handles
 * (fsgpu_sharded_compact / _vacuum) always answer FSGPU_ERR_INVALID_CONFIG: their rows would have to be re-sharded.
 * After a call that changed the slab (fsgpu_index_generation moved) every row id means another row, so
 *   - the library drops what IT derived: the int8 / rotated int8 / 4-bit copies, the measured slab statistics, the MRL views, the
 *     lanes of concurrent callers, the certificate back-off; with FSGPU_INT8_LATENCY_BUILD_NOW in force the copies are rebuilt before
 *     the call returns;
 *   - an fsgpu_allow_bitmap made before is refused (FSGPU_ERR_INVALID_CONFIG): make a new one;
 *   - the CALLER rebuilds what it derived: alignments (fsgpu_alignment_create), hubness tables (fsgpu_index_compute_query_hubness),
 *     k-NN graphs (fsgpu_index_build_knn_graph: after a compaction or a vacuum the rows are renumbered, so every entry of the table
 *     and every list's position names another row — fsgpu_index_update_knn_graph carries the old table over instead of building
 *     it again, with the map fsgpu_index_rewrite_sources hands out), allow bitmaps from fsgpu_index_allow_bitmap_for_hashes, and any fshost_two_tier searcher built over the index (libfshost does
 *     not follow a compaction);
 *   - doc-id pointers handed out by fsgpu_index_doc_id before the call are invalid. */
typedef struct fsgpu_compaction_stats { /* wal::CompactionStats (wal.rs:111) */
    uint64_t main_records_before, wal_records, total_records_after;
    double elapsed_ms;
} fsgpu_compaction_stats;
typedef struct fsgpu_vacuum_stats { /* VacuumStats (lib.rs:726); duration as milliseconds */
    uint64_t records_before, records_after, tombstones_removed, bytes_reclaimed;
    double elapsed_ms;
} fsgpu_vacuum_stats;
/* VectorIndex::compact (lib.rs:2734-2854).  Empty WAL: a no-op that reports {main_before, 0, main_before} — tombstones STAY.  Else the
 * sources are every live main row in row order, then every resident WAL entry in order, stably sorted by (doc_id_hash, doc id bytes);
 * adjacent equal keys collapse to the last (WAL beats main; of two live main duplicates the higher row wins).  Main rows are copied
 * byte for byte (NaN payloads and -0.0 survive); WAL rows are encoded f32 -> f16 round-to-nearest-even on an F16 slab and stored as raw
 * little-endian f32 on an F32 slab.  The WAL is emptied; compaction_gen becomes next_generation (255 -> 1, else +1, lib.rs:6156); the
 * publication nonce, embedder id and revision, dimension and quantization are kept.  Needs a doc-id table (FSVI-opened indexes),
 * else FSGPU_ERR_INVALID_CONFIG.  out may be NULL. */
fsgpu_status fsgpu_index_compact(fsgpu_index *idx, const char *path_or_null, fsgpu_compaction_stats *out);
/* VectorIndex::vacuum (lib.rs:2485-2521).  No rows or no tombstones: a no-op.  Else the live main rows in order, no dedup; the WAL
 * stays resident; compaction_gen is unchanged.  bytes_reclaimed: for an FSVI-opened index the difference of the two FSVI image
 * lengths (layout formula), otherwise the difference in slab bytes.  Works on ANY index (no doc ids needed unless a path is given).
 * On an adopted device slab (fsgpu_index_create_device) the new slab is owned by the library: the caller's slab and live-bitmap
 * buffers are no longer referenced after a vacuum that removed rows and may be freed. */
fsgpu_status fsgpu_index_vacuum(fsgpu_index *idx, const char *path_or_null, fsgpu_vacuum_stats *out);
/* VectorIndex::needs_compaction (lib.rs:2270-2292) with WalConfig's compaction_threshold and compaction_ratio as arguments (the
 * handle keeps no WalConfig; the reference's defaults are 1000 and 0.10): WAL non-empty and (entries >= threshold or, with main
 * rows, entries / record_count >= ratio).  A non-finite ratio means 0.10. */
fsgpu_status fsgpu_index_needs_compaction(fsgpu_index *idx, uint64_t threshold, double ratio, int32_t *out);
/* VectorIndex::needs_vacuum (lib.rs:174, 2464-2475): tombstone_count / record_count > 0.20, strictly. */
fsgpu_status fsgpu_index_needs_vacuum(fsgpu_index *idx, int32_t *out);
uint64_t fsgpu_index_tombstone_count(fsgpu_index *idx); /* VectorIndex::tombstone_count: main rows whose live bit is clear */
uint64_t fsgpu_index_live_count(fsgpu_index *idx);      /* record_count - tombstone_count */
/* Rewrites that changed the slab since the handle was made: starts at 0, +1 per compact / vacuum that was not a no-op. */
uint64_t fsgpu_index_generation(const fsgpu_index *idx);
/* IndexMetadata::compaction_gen (lib.rs:5714-5768): the file header's generation byte, as compact last left it. */
uint32_t fsgpu_index_compaction_gen(const fsgpu_index *idx);
/* Replace the live bitmap (host words, ceil(nrows/64)); NULL = all live. */
fsgpu_status fsgpu_index_set_live_bitmap(fsgpu_index *idx, const uint64_t *live_bitmap);

/* ---- search ---- */
/* Replaces VectorIndex::search_top_k(query, limit, None) (search.rs:192-206 -> :426-494) for nq queries
 * at once: tombstones via the live bitmap, optional per-call allow bitmap (a precomputed SearchFilter,
 * filter.rs:19-56), collect-all when k >= nrows.  query_len must equal the index dimension
 * (else FSGPU_ERR_DIMENSION_MISMATCH, search.rs:1602-1610).  Outputs are [nq,k] row-major, best first;
 * out_counts[q] <= k entries are valid.  No doc-id dedup (see fsgpu_search_hits). */
fsgpu_status fsgpu_search_topk(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                               uint32_t k, const uint64_t *allow_bitmap, uint32_t *out_rows,
                               float *out_scores, uint32_t *out_counts);
/* The same search on the exact f16 kernels, whatever quantised copies the index holds.  fsgpu_search_topk itself answers a LONE
 * unfiltered query (nq = 1, k <= 32) of an index that already holds the int8 copy of its slab — a batched search built it — with ONE
 * certified pass over that copy + an exact re-score of the rows within the proven margin: the rows and f32 score bits of these kernels
 * from half the bytes (a query the certificate does not cover goes to these kernels).  This entry is the checked kernels alone
 * (no coalescing, no int8 pass): what the parity tests compare everything else with. */
fsgpu_status fsgpu_search_topk_exact(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                     const uint64_t *allow_bitmap, uint32_t *out_rows, float *out_scores, uint32_t *out_counts);
/* A SearchFilter is typically built once and reused by many queries (filter.rs:19-56; the filtered search paths search.rs:1114-1255
 * take `Option<&dyn SearchFilter>` per call).  fsgpu_allow_bitmap is the precomputed filter made RESIDENT on the index's device:
 * uploaded once (1.25 MB at 10M rows), then any number of fsgpu_search_topk_filtered / _batched_filtered calls use it without a
 * per-call copy — same hits as fsgpu_search_topk{,_batched} with the same words, same 1/50 selective-gather rule, tombstones still
 * masked at search time.  Concurrent single-query callers that pass the SAME handle share a coalesced batch.  The bitmap belongs to
 * the index it was created for (device and record count are checked). */
typedef struct fsgpu_allow_bitmap fsgpu_allow_bitmap;
fsgpu_status fsgpu_allow_bitmap_create(fsgpu_index *idx, const uint64_t *allow_bitmap, fsgpu_allow_bitmap **out);
void fsgpu_allow_bitmap_destroy(fsgpu_allow_bitmap *filter);
uint64_t fsgpu_allow_bitmap_allowed_rows(const fsgpu_allow_bitmap *filter);
fsgpu_status fsgpu_search_topk_filtered(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                        const fsgpu_allow_bitmap *filter, uint32_t *out_rows, float *out_scores,
                                        uint32_t *out_counts);
fsgpu_status fsgpu_search_topk_batched_filtered(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                                uint32_t k, const fsgpu_allow_bitmap *filter, uint32_t *out_rows,
                                                float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);
/* A filter PER QUERY in one batched, row-level call (no WAL merge, no doc-id dedup: as fsgpu_search_topk_batched).  Query q names
 * filters[filter_of_query[q]], or no filter (-1).  Per query: the rows, f32 score bits and count fsgpu_search_topk_exact returns for
 * that query with that filter's bitmap — (score desc, NaN as -inf, row asc) over the live allowed rows, count = min(k, their number);
 * tombstones are tested when rows are scored, so a soft delete after a filter was made is honoured.  Slots beyond the count are padding.
 * The queries are grouped by filter.  Unfiltered queries ride fsgpu_search_topk_batched; a dense filter's (allowed * 50 >= record count)
 * ride it with that filter's resident bitmap; ALL selective filters' groups (0 < allowed * 50 < record count, the reference's
 * GATHER_SELECTIVITY_DIVISOR, search.rs:1667) share one launch of a segmented gather scan that reads each group's rows from the
 * slab once for all of the group's queries (F16 slab, dense rows, dimension % 8 == 0, k <= 256); an empty filter costs no launch.
 * A selective group outside that shape is answered query by query by the fsgpu_search_topk_filtered path: still exact.
 * *out_fallbacks (optional): those queries plus the ones the batched groups handed to the exact kernels.
 * Refused before anything is launched: query_len != dimension (FSGPU_ERR_DIMENSION_MISMATCH); a filter_of_query entry < -1 or
 * >= nfilters, a filter of another index or from before a compact / vacuum (FSGPU_ERR_INVALID_CONFIG).  fsgpu_index handles only. */
fsgpu_status fsgpu_search_topk_batched_multi_filtered(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                                      uint32_t k, const fsgpu_allow_bitmap *const *filters, uint32_t nfilters,
                                                      const int32_t *filter_of_query, uint32_t *out_rows, float *out_scores,
                                                      uint32_t *out_counts, uint32_t *out_fallbacks);
/* ... with the queries and the three outputs in device memory, enqueued on `hip_stream`, which is synchronised before the call
 * returns (as fsgpu_search_topk_batched_device does); filters and filter_of_query stay host arrays. */
fsgpu_status fsgpu_search_topk_batched_multi_filtered_device_queries(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                                                     uint32_t query_len, uint32_t k,
                                                                     const fsgpu_allow_bitmap *const *filters, uint32_t nfilters,
                                                                     const int32_t *filter_of_query, uint32_t *out_rows_dev,
                                                                     float *out_scores_dev, uint32_t *out_counts_dev, void *hip_stream,
                                                                     uint32_t *out_fallbacks);
/* The ascending row ids of a filter's set bits (bits past the record count ignored), as the DEVICE built them from the resident
 * bitmap — popcount per 64-bit word, exclusive scan, expand; built at first use and kept on the handle.  *out_n = their number;
 * the first min(cap, *out_n) are copied to out_rows. */
fsgpu_status fsgpu_allow_bitmap_rows(const fsgpu_allow_bitmap *filter, uint32_t *out_rows, uint64_t cap, uint64_t *out_n);
/* Queries fsgpu_search_topk_batched_multi_filtered has answered so far, by path: the gather scan, a dense group's masked pass, no
 * filter, the per-query fallback of a selective group (any pointer may be null). */
fsgpu_status fsgpu_index_multi_filter_stats(fsgpu_index *idx, uint64_t *gathered, uint64_t *scanned, uint64_t *unfiltered,
                                            uint64_t *fallbacks);
/* Same, all pointers device-resident, enqueued on `hip_stream` (a hipStream_t), no host sync. */
fsgpu_status fsgpu_search_topk_device(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                      uint32_t query_len, uint32_t k, const uint64_t *allow_bitmap_dev,
                                      uint32_t *out_rows_dev, float *out_scores_dev, uint32_t *out_counts_dev,
                                      void *hip_stream);
/* Throughput form of fsgpu_search_topk for large query batches: groups of 64 queries share ONE pass over the
 * slab on the matrix cores (f16-rounded queries, v_mfma_f32_16x16x32_f16); rows that could reach the top k under a
 * proven error bound are re-scored in the reference's exact order, so rows and score bits are IDENTICAL to
 * fsgpu_search_topk.  Queries the batched path cannot certify (k > 64, unsupported dimension, margin overflow) are
 * answered by the exact kernels; *out_fallbacks (optional) counts them.  The _device form synchronises hip_stream. */
/* The filter those passes score with is chosen per index (FSGPU_FILTER_AUTO): batches of 16 queries and more are
 * filtered on an int8 copy of the slab (built on first use, half an F16 slab's size again, a quarter of an F32 slab's;
 * v_mfma_i32_16x16x64_i8: half the bytes and half the matrix instructions per f16 row) under a bound measured from the slab and each
 * query (mfma_scan.hip, prepare_queries_i8_filter_kernel); queries whose margin lets too many rows through are re-filtered on the f16
 * slab, and an index where that happens to more than 1/8 of a batch twice in a row (or that has no room for the copy) stays with the
 * f16 filter.  Either way the emitted rows and score bits are the exact search's.
 * An F32 slab (Quantization::F32) has the int8 filter and no f16 one: its candidates are re-scored from the f32 rows in
 * dot_product_f32_bytes_f32's order, queries the int8 filter cannot certify go straight to the exact f32 kernels (counted in
 * *out_fallbacks, not as re-filtered), and FSGPU_FILTER_F16 — or an index that gave the int8 filter up — means those kernels for the
 * whole batch.  The int8 two-pass searches stay F16-only, as in the reference (search.rs:579-585). */
#define FSGPU_FILTER_AUTO 0
#define FSGPU_FILTER_F16 1
#define FSGPU_FILTER_INT8 2
fsgpu_status fsgpu_index_set_batched_filter(fsgpu_index *idx, int32_t filter);
/* The int8 filter's copy of a slab WITH OUTLIER CHANNELS (a few dimensions carrying most of every row's norm, as trained embedding
 * models have) is built from ROTATED rows: one corpus-wide int8 scale (simd.rs:1865-1886) spends the int8 range on those channels, and
 * the filter's proven margin — fixed in integer units — is then several times wider in cosine units than it has to be.  Dot products
 * are invariant under an orthogonal map: the filter scores quantised R x against quantised R q (R fixed, random, applied in f64 and
 * rounded once to f32; what that adds to the proven bound is 2^-24-sized), and the exact re-score that decides rows and score bits never
 * sees the rotation.  AUTO (default): rotate when the slab's largest |element| x sqrt(dim) exceeds 9 x its largest row norm — decided
 * once, when the copy is built (first batched search).  The reference has no counterpart (its int8 slab serves the two-pass search,
 * which keeps the reference's own quantisation here too).  Takes effect for a copy that is not built yet. */
#define FSGPU_ROTATION_AUTO 0
#define FSGPU_ROTATION_OFF 1
#define FSGPU_ROTATION_ON 2
fsgpu_status fsgpu_index_set_filter_rotation(fsgpu_index *idx, int32_t mode);
int32_t fsgpu_index_filter_rotated(fsgpu_index *idx); /* 1: the filter's copy of this index is the rotated one */
/* Latency form of the same idea: with this set, unfiltered fsgpu_search_topk calls of up to 16 queries (k <= 64) are answered
 * through the int8 filter + exact re-score as well — the pass streams half the bytes, rows and score bits unchanged; the int8 copy is
 * built at the first such call.  A lone query (k <= 32) takes ONE certified pass: every block of the int8 scan keeps its 32 best entries,
 * the rows within the proven margin of the k-th are re-scored from the f16 slab, and the answer stands when no block can have dropped a
 * row within that margin (one query at 10M x 384: p50 0.67 ms against 1.26 ms; 1M x 384: 0.126 against 0.161); an uncertified query
 * takes the staged path.  Off by default: fsgpu_search_topk then takes the certified pass only for a lone query of an index whose int8
 * copy a batched search has already built (see fsgpu_search_topk_exact above) and never builds the copy itself; the two-tier host
 * (libfshost) sets it on the quality tier.
 * enabled = FSGPU_INT8_LATENCY_BUILD_NOW: on, and the int8 copy + its statistics are built before the call returns (index-build work,
 * ~4 ms per GB of slab), so that the latency of the first lone query does not depend on what was searched before it. */
#define FSGPU_INT8_LATENCY_BUILD_NOW 2
fsgpu_status fsgpu_index_set_int8_latency(fsgpu_index *idx, int32_t enabled);
/* Queries the int8 filter has taken so far, how many of them it handed on to the f16 filter, and whether the index still
 * uses it (any pointer may be null). */
fsgpu_status fsgpu_index_batched_filter_stats(fsgpu_index *idx, uint64_t *int8_queries, uint64_t *refiltered_f16,
                                              int32_t *int8_active);
/* The int8 filter's certificate, for inspection (tests/test_gpu_int8_filter.py checks it against float64 arithmetic): per
 * query the bound out_delta[q] >= |int8 score - exact score * slab scale * query scale| over every row (< 0: the query
 * cannot be certified and goes to the f16 filter — on an F32 slab, to the exact kernels), the scales 127 / max|q| and 127 / max|x|, the quantised queries
 * [nq, dim] and the int8 slab [rows, dim] (any output may be null).  Builds the int8 copy if it does not exist yet.  Serves F16
 * and F32 slabs with dense rows (tests/test_gpu_f32_batched.py checks the F32 form the same way). */
fsgpu_status fsgpu_index_int8_filter_bound(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                           float *out_delta, float *out_query_scale, float *out_slab_scale,
                                           int8_t *out_queries_i8, int8_t *out_slab_i8);
fsgpu_status fsgpu_search_topk_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                       uint32_t k, const uint64_t *allow_bitmap, uint32_t *out_rows, float *out_scores,
                                       uint32_t *out_counts, uint32_t *out_fallbacks);
fsgpu_status fsgpu_search_topk_batched_device(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                              uint32_t query_len, uint32_t k, const uint64_t *allow_bitmap_dev,
                                              uint32_t *out_rows_dev, float *out_scores_dev, uint32_t *out_counts_dev,
                                              void *hip_stream, uint32_t *out_fallbacks);
/* Shard-local search for the multi-GPU path (the reference partitions the same way per
 * rayon chunk, search.rs:1020-1035): like fsgpu_search_topk_device but the result stays PACKED,
 * out_packed_dev[q*k+i] = (f32 score bits << 32) | global row, best first, ~0ull padding — one
 * 8-byte word per hit, ready for an RCCL all-gather.  k <= 256, dim % 8 == 0. */
fsgpu_status fsgpu_search_topk_packed_device(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                             uint32_t query_len, uint32_t k, const uint64_t *allow_bitmap_dev,
                                             uint64_t *out_packed_dev, void *hip_stream);
/* Batched (matrix-core) form of fsgpu_search_topk_packed_device: same packed output, same exact results, 64 queries
 * per pass.  Synchronises hip_stream. */
fsgpu_status fsgpu_search_topk_batched_packed_device(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                                     uint32_t query_len, uint32_t k, const uint64_t *allow_bitmap_dev,
                                                     uint64_t *out_packed_dev, void *hip_stream, uint32_t *out_fallbacks);
/* The batched searches in two halves, for a caller that keeps its GPU fed: _begin enqueues the WHOLE search on hip_stream and returns
 * a ticket without waiting (0 / 1: two may be outstanding per index); _end waits for that search's last kernel — an event, not the
 * stream, which may already hold the caller's next search —, reads the per-query verdicts and answers the rare uncertified query with
 * the exact kernels, exactly as the blocking forms do at their end.  Outputs as in fsgpu_search_topk_batched_device (rows / scores /
 * counts, each may be null) plus out_packed_dev as in the packed form (may be null); the queries and every output stay the caller's
 * until _end.  Between a _begin and its _end the index may begin ONE more search; blocking calls on the same index are allowed:
 * a batched search on another stream than an outstanding ticket's is ordered behind that ticket's last kernel on the device (all
 * batched searches of an index share one set of workspaces), on the same stream it queues behind by itself.  Calls that CHANGE
 * the index (fsgpu_index_set_live_bitmap, _soft_delete, _wal_append) are refused with FSGPU_ERR_INVALID_CONFIG while a ticket is
 * outstanding.  The per-rank loop of `bench.py --gpus N` (frankensearch_amd/sharded.py) runs on these: the ~50 us between
 * one blocking call's wake-up and the next call's first kernel were a tenth of a 1.25M-row shard's step.  No reference counterpart
 * (the reference's scan is synchronous CPU code, search.rs:1013-1080). */
fsgpu_status fsgpu_search_topk_batched_device_begin(fsgpu_index *idx, const float *queries_dev, uint32_t nq, uint32_t query_len,
                                                    uint32_t k, const uint64_t *allow_bitmap_dev, uint32_t *out_rows_dev,
                                                    float *out_scores_dev, uint32_t *out_counts_dev, uint64_t *out_packed_dev,
                                                    void *hip_stream, int32_t *out_ticket);
fsgpu_status fsgpu_search_topk_batched_device_end(fsgpu_index *idx, int32_t ticket, uint32_t *out_fallbacks);
/* ... the same, also reporting how many queries were ANSWERED IN THE END HALF — by the exact kernels (*out_fallbacks) or by the f16
 * filter after the int8 filter handed them on (re-filtered: certified, not a fallback).  Their hits are written by work enqueued on
 * hip_stream inside this call: a caller that chained work to the last kernel of _begin (a shard's all-gather behind an event recorded
 * right after _begin returned) must chain it again when *out_late_answers != 0. */
fsgpu_status fsgpu_search_topk_batched_device_end_late(fsgpu_index *idx, int32_t ticket, uint32_t *out_fallbacks,
                                                       uint32_t *out_late_answers);
/* One-shot hook for the NEXT batched search on this handle: `fn(ctx)` is called on the calling thread once every kernel of
 * that search is enqueued and before the call blocks on its stream (it has to read the certificate flags back).  A launcher
 * that pipelines steps uses the window to enqueue the PREVIOUS step's exchange (all-gather + merge on another stream), so
 * that host work runs under the scan instead of between two scans.  The hook must not call into this handle.  A search that
 * leaves the matrix-core path (odd shapes) returns without calling it; the hook is cleared either way. */
typedef void (*fsgpu_after_enqueue_fn)(void *ctx);
fsgpu_status fsgpu_index_set_after_enqueue_hook(fsgpu_index *idx, fsgpu_after_enqueue_fn fn, void *ctx);
/* Merge of gathered packed lists = merge_partial_heaps + resolve_hits sort (search.rs:1704-1720,1493-1501)
 * across shards: entry (q, l, i) is lists_dev[q*q_stride + l*l_stride + i]; selects the k best per query
 * under the reference order.  For an all-gather result laid out [nlists][nq][list_len]:
 * q_stride = list_len, l_stride = nq*list_len. */
fsgpu_status fsgpu_merge_topk_device(int32_t device, const uint64_t *lists_dev, uint32_t nq, uint32_t nlists,
                                     uint32_t list_len, uint64_t q_stride, uint64_t l_stride, uint32_t k,
                                     uint32_t *out_rows_dev, float *out_scores_dev, uint32_t *out_counts_dev,
                                     void *hip_stream);
/* search_top_k_classified (search.rs:227-261): validates the query (non-finite -> INVALID_CONFIG),
 * reports the ZeroSignalReason, then searches one query (through fsgpu_search_hits when the index has a doc-id
 * table, so resident WAL entries count; row-level otherwise). */
fsgpu_status fsgpu_search_topk_classified(fsgpu_index *idx, const float *query, uint32_t query_len, uint32_t k,
                                          uint32_t *out_rows, float *out_scores, uint32_t *out_count,
                                          int32_t *zero_signal);
/* search_top_k + scan_wal + resolve_hits (search.rs:426-494, 1449-1475, 1493-1558) for FSVI-opened indexes:
 * GPU top-k of the main rows, merge of the resident WAL entries (dot_product_f32_f32 on the host, as in the
 * reference), WAL shadowing, post-top-k doc-id dedup (first = best wins).  WAL hits report the virtual row
 * record_count + wal index.  out_* hold up to k entries. */
fsgpu_status fsgpu_search_hits(fsgpu_index *idx, const float *query, uint32_t query_len, uint32_t k,
                               uint32_t *out_rows, float *out_scores, uint32_t *out_count);
/* fsgpu_search_hits for nq queries: out_rows / out_scores [nq, k], out_counts [nq] (<= k; may be shorter after shadowing / dedup,
 * exactly as the per-query call).  WAL hits report the virtual row record_count + wal index.  The main rows come from the batched
 * matrix-core search and stay in device memory; the resident WAL is scored by wal_topk_kernel against a device mirror of its
 * embeddings (dot_product_f32_f32, the handle's hreduce mode) and resolve_hits_kernel merges, shadows and dedups by doc-id CLASS
 * (doc ids are compared as bytes once, when the tables are built; any change of the WAL, the tombstones or the slab rebuilds them).
 * Rows, score bits and counts equal the per-query call's.  *out_fallbacks (may be NULL) counts the queries answered through the
 * per-query call — ALL of them for k = 0, k > 256, record_count + wal count >= 2^32, a dimension whose single query does not fit the
 * WAL kernel's LDS (beyond ~32,000), and a handle whose main rows are not its own slab from row 0 (the catalog of a row-sharded
 * index, a shard with a row base) — else those the batched search itself answered by fallback (their main rows came from the exact
 * kernels: same bits; the WAL and resolve steps still ran on the device).  A failed kernel launch is FSGPU_ERR_DEVICE, never a
 * fallback.  An index without a doc-id table is FSGPU_ERR_INVALID_CONFIG, as in fsgpu_search_hits.  Refused while a begun batched
 * search is outstanding. */
fsgpu_status fsgpu_search_hits_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                       uint32_t *out_rows, float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);
/* the same with the queries in device memory (where fsgpu_bert_embed_device / fsgpu_m2v_embed_device left them); host results */
fsgpu_status fsgpu_search_hits_batched_device_queries(fsgpu_index *idx, const float *queries_dev, uint32_t nq, uint32_t query_len,
                                                      uint32_t k, uint32_t *out_rows, float *out_scores, uint32_t *out_counts,
                                                      uint32_t *out_fallbacks);
/* search_top_k_int8_two_pass / _4bit_two_pass (search.rs:514-661, 876-946) for a batch on an index WITH a doc-id table: with a
 * resident WAL the reference falls back to the exact search (search.rs:579-585) -> fsgpu_search_hits_batched; otherwise the
 * row-level batched two-pass, then resolve_hits' dedup on the device.  bits = 8 or 4.  Identical per query to
 * fsgpu_search_topk_{int8,4bit}_two_pass. */
fsgpu_status fsgpu_search_hits_two_pass_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                                uint32_t candidate_multiplier, uint32_t bits, uint32_t *out_rows, float *out_scores,
                                                uint32_t *out_counts, uint32_t *out_fallbacks);
/* VectorIndex::search_top_k_int8_two_pass(query, k, candidate_multiplier) (search.rs:514-661) — the reference's
 * production default for the fast tier (two_tier.rs:1332-1337, multiplier 3): pass 1 scans a lazily built int8
 * slab (one corpus-wide max-abs scale, simd.rs:1865-1886) with the integer-exact dot and keeps the top
 * max(min(k*mult, N), min(k, N)) rows under (int score desc, row asc); pass 2 re-scores those rows with the exact
 * f16 dot and selects k under the usual order; doc-id dedup when the index has a doc-id table.  Falls back to the
 * exact search when a WAL is resident.  Halves the HBM bytes of a pass (N*dim). */
fsgpu_status fsgpu_search_topk_int8_two_pass(fsgpu_index *idx, const float *query, uint32_t query_len, uint32_t k,
                                             uint32_t candidate_multiplier, uint32_t *out_rows, float *out_scores,
                                             uint32_t *out_count);
/* Batched search_top_k_int8_two_pass: nq queries share each pass over the int8 slab (int8 MFMA, exact integer
 * scores: the k*candidate_multiplier candidates of every query are exactly the reference's), then the exact f16 rescore
 * and the best-first selection of k.  Outputs as fsgpu_search_topk ([nq, k] rows / scores, [nq] counts).  Row-level
 * results: indexes with a doc-id table, a resident WAL, k = 0 or shapes the matrix-core kernel does not cover are
 * answered query by query through fsgpu_search_topk_int8_two_pass (counted in *out_fallbacks, may be NULL). */
fsgpu_status fsgpu_search_topk_int8_two_pass_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t candidate_multiplier, uint32_t *out_rows,
                                                     float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);

/* VectorIndex::search_top_k_4bit_two_pass (crates/frankensearch-index/src/search.rs:876-946): pass 1 over a packed
 * signed-4-bit slab (dim/2 bytes per vector, one corpus-wide scale 7/max_abs, simd.rs:2153-2215; exact integer nibble
 * dot, simd.rs:1338-1556) keeps the top k*candidate_multiplier, pass 2 re-scores them with the exact f16 dot.  Same
 * arguments, outputs and fallbacks (WAL resident, k = 0, empty index -> exact search) as the int8 variant. */
fsgpu_status fsgpu_search_topk_4bit_two_pass(fsgpu_index *idx, const float *query, uint32_t query_len, uint32_t k,
                                             uint32_t candidate_multiplier, uint32_t *out_rows, float *out_scores,
                                             uint32_t *out_count);
/* Batched search_top_k_4bit_two_pass: as fsgpu_search_topk_int8_two_pass_batched, with the reference's 4-bit quantisers
 * (slab scale 7/max_abs, pack_4bit_query).  The nibble dot is an exact integer, so the levels are kept one per byte (built on
 * first use, rows x dim bytes) and run through the same int8 matrix-core pass — which is bound by matrix instructions, not
 * by bytes — giving exactly the reference's k*candidate_multiplier candidates; then the exact f16 rescore. */
fsgpu_status fsgpu_search_topk_4bit_two_pass_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t candidate_multiplier, uint32_t *out_rows,
                                                     float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);
/* VectorIndex::dot_query_at (lib.rs:3229-3239) over a row list, as used by
 * TwoTierIndex::quality_scores_for_hits (two_tier.rs:1566-1631).  rows are global ids. */
fsgpu_status fsgpu_gather_dot(fsgpu_index *idx, const float *query, uint32_t query_len, const uint32_t *rows,
                              uint32_t n, float *out_scores);

/* ---- row-sharded index over the GPUs of one node ---- */
/* The reference's only partitioning is scan_parallel's contiguous row chunks merged by merge_partial_heaps
 * (crates/frankensearch-index/src/search.rs:1013-1036,1704-1720).  A sharded handle is the same shape across GPUs, inside the
 * library, so that the host makes ONE call per search: shard r (on devices[r]) owns the contiguous rows
 * [r*ceil(N/ndev), ...) and reports global row ids; queries are replicated; each shard scans on its own stream; one
 * ncclAllGather (RCCL over xGMI, nq*k*8 bytes per shard; issued for all shards inside one ncclGroupStart/End from the calling
 * thread, on per-shard exchange streams behind an event of the scan — no host wait between scan, all-gather and merge) gathers
 * the packed per-shard top-k lists and the root device merges them under the reference order.  Results are identical to an
 * unsharded index over the same rows, for every entry point below. */
typedef struct fsgpu_sharded fsgpu_sharded;
#define FSGPU_EXCHANGE_AUTO 0      /* RCCL when the devices are distinct and librccl.so.1 loads, else peer copies */
#define FSGPU_EXCHANGE_RCCL 1      /* ncclCommInitAll + ncclAllGather; creation fails if RCCL cannot be used */
#define FSGPU_EXCHANGE_PEER_COPY 2 /* device-to-device copies into the root's gather buffer (also: several shards on ONE
                                      device, a rehearsal of the N-way path on fewer GPUs — RCCL wants one rank per device) */
/* VectorIndex::open for a host slab of nrows x dim little-endian f16 rows, split over devices[0..ndev).  live_bitmap as in
 * fsgpu_index_create (bit r = global row r is live; NULL = all live). */
fsgpu_status fsgpu_sharded_create(const int32_t *devices, uint32_t ndev, uint32_t dim, uint64_t nrows, const void *slab_f16_le,
                                  const uint64_t *live_bitmap, int32_t exchange, fsgpu_sharded **out);
/* Zero-copy variant: shard r adopts (does not free) shard_rows[r] rows already resident on devices[r] (shard_live_dev and its
 * entries may be NULL); global row ids follow the order of the shards. */
fsgpu_status fsgpu_sharded_create_device(const int32_t *devices, uint32_t ndev, uint32_t dim, const uint64_t *shard_rows,
                                         const void *const *shard_slabs_dev, const uint64_t *const *shard_live_dev,
                                         int32_t exchange, fsgpu_sharded **out);
/* Hybrid layout (round 5): ndev = query_groups x row shards.  Device r holds row shard r % (ndev / query_groups) — every row shard is
 * resident once per group (288 GB per GPU hold a 10M x 384 slab many times over) — and scans it for the queries of group
 * r / (ndev / query_groups), a contiguous 1/query_groups of the batch.  A shard's step has a fixed part that does not shrink with its
 * rows (sample, selections, launches): 2 groups x 4 row shards pay it over 2.5M rows and half the queries per device where 8 row
 * shards pay it over 1.25M rows and every query.  Same results as the unsharded index; ONE all-gather over all devices, one merge per
 * group.  The reference partitions rows only (scan_parallel, search.rs:1013-1036); splitting the QUERY batch as well has no
 * counterpart there because its callers issue one query at a time.  query_groups = 1 is fsgpu_sharded_create{,_device} /
 * fsgpu_sharded_open_fsvi.  _create_device_grouped: shard_rows / slabs / live per DEVICE; shard_rows[r] must equal
 * shard_rows[r % row shards]. */
fsgpu_status fsgpu_sharded_create_grouped(const int32_t *devices, uint32_t ndev, uint32_t query_groups, uint32_t dim, uint64_t nrows,
                                          const void *slab_f16_le, const uint64_t *live_bitmap, int32_t exchange, fsgpu_sharded **out);
fsgpu_status fsgpu_sharded_create_device_grouped(const int32_t *devices, uint32_t ndev, uint32_t query_groups, uint32_t dim,
                                                 const uint64_t *shard_rows, const void *const *shard_slabs_dev,
                                                 const uint64_t *const *shard_live_dev, int32_t exchange, fsgpu_sharded **out);
uint32_t fsgpu_sharded_query_groups(const fsgpu_sharded *idx);
uint32_t fsgpu_sharded_row_shards(const fsgpu_sharded *idx);
void fsgpu_sharded_destroy(fsgpu_sharded *idx);
uint64_t fsgpu_sharded_record_count(const fsgpu_sharded *idx);
uint32_t fsgpu_sharded_dimension(const fsgpu_sharded *idx);
uint32_t fsgpu_sharded_shard_count(const fsgpu_sharded *idx); /* devices: query groups x row shards */
int32_t fsgpu_sharded_exchange_mode(const fsgpu_sharded *idx); /* FSGPU_EXCHANGE_RCCL or FSGPU_EXCHANGE_PEER_COPY, as chosen */
int32_t fsgpu_sharded_device(const fsgpu_sharded *idx, uint32_t shard); /* the HIP device of a shard (shard 0 = the root: merges, takes queries_dev) */
fsgpu_status fsgpu_sharded_shard_range(const fsgpu_sharded *idx, uint32_t shard, uint64_t *row_lo, uint64_t *row_hi);
fsgpu_status fsgpu_sharded_set_hreduce(fsgpu_sharded *idx, int32_t mode);
/* VectorIndex::search_top_k(query, limit, None) for nq host queries over all shards (exact kernels); outputs as
 * fsgpu_search_topk.  k <= 256 and dim % 8 == 0 (the packed lists of the fused tiers are what travels). */
fsgpu_status fsgpu_sharded_search_topk(fsgpu_sharded *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                       uint32_t *out_rows, float *out_scores, uint32_t *out_counts);
/* Same answers through the matrix-core batched path of every shard (fsgpu_search_topk_batched); *out_fallbacks (optional) sums
 * the per-shard exact fallbacks. */
fsgpu_status fsgpu_sharded_search_topk_batched(fsgpu_sharded *idx, const float *queries, uint32_t nq, uint32_t query_len,
                                               uint32_t k, uint32_t *out_rows, float *out_scores, uint32_t *out_counts,
                                               uint32_t *out_fallbacks);
/* The general form: VectorIndex::search_top_k(query, limit, filter) (search.rs:192-206) and the two-pass searches
 * (search.rs:514-661, 876-946) on one object.
 *   mode  FSGPU_SHARDED_EXACT / _BATCHED: the exact kernels / the matrix-core batched path of every shard; allow_bitmap (optional)
 *         is the index-wide precomputed SearchFilter (bit r = global row r may be returned, filter.rs:19-56), split per shard
 *         like the live bitmap.
 *         FSGPU_SHARDED_INT8_TWO_PASS / _4BIT_TWO_PASS: search_top_k_int8_two_pass / search_top_k_4bit_two_pass for the batch.
 *         Every shard quantises with the ONE corpus-wide scale of the reference (simd.rs:1865-1886: max-abs over the whole slab —
 *         an ncclAllReduce(max) of 4 bytes over the shards, once per index) and hands its k*candidate_multiplier pass-1
 *         candidates to the root as (pass-1 entry, exact entry) pairs; the root takes the corpus-wide k*candidate_multiplier
 *         best by the pass-1 order — exactly the unsharded candidate set — and the k best of those by the exact order.
 *         k*candidate_multiplier <= 256, shards*k*candidate_multiplier <= 1024, no filter.
 * fsgpu_sharded_search = begin + end, both on the calling thread (no worker threads inside the handle): begin ENQUEUES every
 * shard's scan on that shard's stream — the batched and two-pass searches through their begin halves, so no host wait sits between
 * one search's last kernel and the next one's first — and the exchange + merge behind them; end waits for that one search, reads the
 * shards' verdicts and, only if a shard had to answer an uncertified query late, sends the corrected lists through the exchange again.
 * Two searches may be in flight per handle (end them in order), so the exchange and merge of one run underneath the scan of the next.
 * A LONE query (nq = 1, host pointer, no filter, mode EXACT or a two-pass mode) takes the shards' latency lanes instead (certified
 * int8 pass with fsgpu_sharded_set_int8_latency, two-pass lane): every shard of one query group answers into its own pinned block,
 * all begun before any is waited for, and the calling thread merges the short lists — merge_partial_heaps on the host, where the
 * reference runs it (search.rs:1704-1720); no collective, no merge launch, no D2H copy. */
#define FSGPU_SHARDED_EXACT 0
#define FSGPU_SHARDED_BATCHED 1
#define FSGPU_SHARDED_INT8_TWO_PASS 2
#define FSGPU_SHARDED_4BIT_TWO_PASS 3
typedef struct fsgpu_sharded_request {
    const float *queries;          /* [nq, query_len] host */
    uint32_t nq, query_len, k;
    int32_t mode;
    uint32_t candidate_multiplier; /* two-pass modes (0 counts as 1, as in the reference) */
    const uint64_t *allow_bitmap;  /* ceil(N/64) words or NULL */
    const float *queries_dev;      /* NULL, or the queries already RESIDENT on devices[0] (an encoder's device output,
                                    * fsgpu_bert_embed_device): `queries` is then ignored — no staging, no H2D copy; the other shards
                                    * fetch them from the root peer to peer (xGMI).  Must stay unchanged until the search has ended. */
} fsgpu_sharded_request;
fsgpu_status fsgpu_sharded_search(fsgpu_sharded *idx, const fsgpu_sharded_request *request, uint32_t *out_rows, float *out_scores,
                                  uint32_t *out_counts, uint32_t *out_fallbacks);
/* The batch's queries resident in PARTS on several devices — data-parallel encoders ("Encoders: data-parallel over the
 * query batch"): part p holds part_counts[p] consecutive queries on device part_devices[p] (fsgpu_bert_embed_device of that device's
 * encoder); request->queries / queries_dev are ignored, the counts add up to request->nq.  Every device fetches the slice of its query
 * group peer to peer over xGMI (in place when the slice is one part on that very device).  Blocking (begin + end). */
fsgpu_status fsgpu_sharded_search_parts(fsgpu_sharded *idx, const fsgpu_sharded_request *request, const float *const *parts_dev,
                                        const uint32_t *part_counts, const int32_t *part_devices, uint32_t n_parts, uint32_t *out_rows,
                                        float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);
/* fsgpu_index_set_int8_latency for every shard: lone EXACT queries take ONE certified pass over the shard's int8 copy (built here,
 * from the corpus-wide scale) + exact re-score instead of the exact kernel's pass over the f16 rows — same rows and score bits, half
 * the bytes.  Off by default. */
fsgpu_status fsgpu_sharded_set_int8_latency(fsgpu_sharded *idx, int32_t enabled);
fsgpu_status fsgpu_sharded_search_begin(fsgpu_sharded *idx, const fsgpu_sharded_request *request, uint64_t *out_ticket);
fsgpu_status fsgpu_sharded_search_end(fsgpu_sharded *idx, uint64_t ticket, uint32_t *out_rows, float *out_scores,
                                      uint32_t *out_counts, uint32_t *out_fallbacks);
/* Dynamic batching of concurrent callers on a sharded handle (as fsgpu_index_set_coalescing): fsgpu_sharded_search calls with
 * nq = 1, k <= 64, no allow bitmap and mode EXACT or INT8_TWO_PASS that are in flight together ride ONE search of the shards (more
 * than four exact callers take the BATCHED mode — the same rows and score bits; two-pass callers one two-pass batch with their
 * multiplier).  max_batch = 0 turns it off (the default). */
fsgpu_status fsgpu_sharded_set_coalescing(fsgpu_sharded *idx, uint32_t max_batch, uint32_t max_wait_us);
fsgpu_status fsgpu_sharded_coalescing_stats(fsgpu_sharded *idx, uint64_t *batches, uint64_t *requests);
/* the corpus-wide max-abs the shards' int8 / 4-bit copies are built from (0 before the first two-pass search) */
float fsgpu_sharded_quant_scale_max(const fsgpu_sharded *idx);
/* VectorIndex::open (lib.rs:1747-1909) of an FSVI v1 file (F16 or F32 slab), rows split over the devices.  The handle keeps the
 * record table, the doc-id strings and the tombstone flags, so the doc-id level calls below work as on fsgpu_index.  On an F32 file
 * the two-pass modes are refused (FSGPU_ERR_INVALID_CONFIG, "two-pass searches need an F16 slab"); the exact and batched modes serve it. */
fsgpu_status fsgpu_sharded_open_fsvi(const char *path, const int32_t *devices, uint32_t ndev, int32_t exchange, fsgpu_sharded **out);
fsgpu_status fsgpu_sharded_open_fsvi_grouped(const char *path, const int32_t *devices, uint32_t ndev, uint32_t query_groups,
                                             int32_t exchange, fsgpu_sharded **out);
/* index-wide tombstone bitmap (bit r = global row r is live; NULL = all live), split per shard */
fsgpu_status fsgpu_sharded_set_live_bitmap(fsgpu_sharded *idx, const uint64_t *live_bitmap);
/* soft_delete / append / doc ids / search_top_k with the resident WAL, shadowing and doc-id dedup (fsgpu_index_soft_delete,
 * fsgpu_index_wal_append, fsgpu_index_doc_id, fsgpu_search_hits): handles opened with fsgpu_sharded_open_fsvi */
fsgpu_status fsgpu_sharded_soft_delete(fsgpu_sharded *idx, const char *doc_id, uint32_t doc_id_len, int32_t *out_deleted);
fsgpu_status fsgpu_sharded_wal_append(fsgpu_sharded *idx, const char *doc_id, uint32_t doc_id_len, const float *vector,
                                      uint32_t vector_len);
/* VectorIndex::compact / vacuum under a row-sharded handle: always FSGPU_ERR_INVALID_CONFIG (re-sharding is not built). */
fsgpu_status fsgpu_sharded_compact(fsgpu_sharded *idx, const char *path_or_null, fsgpu_compaction_stats *out);
fsgpu_status fsgpu_sharded_vacuum(fsgpu_sharded *idx, const char *path_or_null, fsgpu_vacuum_stats *out);
uint64_t fsgpu_sharded_wal_record_count(const fsgpu_sharded *idx);
fsgpu_status fsgpu_sharded_doc_id(const fsgpu_sharded *idx, uint32_t row, const char **out_ptr, uint32_t *out_len);
fsgpu_status fsgpu_sharded_search_hits(fsgpu_sharded *idx, const float *query, uint32_t query_len, uint32_t k, uint32_t *out_rows,
                                       float *out_scores, uint32_t *out_count);
/* dot_query_at over global row ids, each routed to the shard that owns it (fsgpu_gather_dot) */
fsgpu_status fsgpu_sharded_gather_dot(fsgpu_sharded *idx, const float *query, uint32_t query_len, const uint32_t *rows, uint32_t n,
                                      float *out_scores);

/* ---- index build helpers ---- */
/* VectorIndexWriter::write_record + finish for FSVI v1 (crates/frankensearch-index/src/lib.rs:3637-3672, 3752-3943): every
 * vector must be finite with a usable norm and every doc id fit in u16 bytes (else FSGPU_ERR_INVALID_CONFIG, nothing
 * written); records are stably sorted by (FNV-1a(doc_id), doc_id) and written as header (CRC32) | 16-byte records | string
 * table | pad to 64 | little-endian f16 slab (f32 -> f16 round-to-nearest-even on `device`).  The bytes equal the
 * reference writer's for the same input.  doc_id_lens may be NULL (NUL-terminated ids).  n may exceed the GPU grid limit
 * only in theory (n < 2^31). */
fsgpu_status fsgpu_fsvi_write(const char *path, const char *embedder_id, const char *embedder_revision, uint32_t dim,
                              uint64_t n, const char *const *doc_ids, const uint32_t *doc_id_lens, const float *vectors,
                              uint8_t compaction_gen, int32_t device);

/* The same writer for either Quantization (lib.rs:203-208): quantization 1 = F16 (as above), 0 = F32 (rows stored as raw
 * little-endian f32, write_vector_slab lib.rs:6017-6024).  F32 files open and search like F16 ones (dot_product_f32_bytes_f32,
 * simd.rs:581-702), through the general path only: F16 is the reference's default and the accelerated format. */
fsgpu_status fsgpu_fsvi_write_quant(const char *path, const char *embedder_id, const char *embedder_revision, uint32_t dim,
                                    uint64_t n, const char *const *doc_ids, const uint32_t *doc_id_lens,
                                    const float *vectors, uint8_t compaction_gen, int32_t device, uint8_t quantization);

/* encode_f32_to_f16_extend (simd.rs:2245-2305): f32 -> f16 round-to-nearest-even on the GPU. */
fsgpu_status fsgpu_encode_f32_to_f16(int32_t device, const float *src, uint64_t n, uint16_t *dst);
/* f16 -> f32 widen (simd.rs:63-94), exposed for the exhaustive 65,536-pattern parity test. */
fsgpu_status fsgpu_widen_f16_to_f32(int32_t device, const uint16_t *src, uint64_t n, float *dst);

/* ---- Model2Vec (potion) ---- */
/* Model2VecEmbedder (embed/src/model2vec_embedder.rs:55-58): table is [vocab,dim] f32 row-major (host). */
fsgpu_status fsgpu_m2v_create(int32_t device, const float *table, uint32_t vocab, uint32_t dim, fsgpu_m2v **out);
void fsgpu_m2v_destroy(fsgpu_m2v *m);
uint32_t fsgpu_m2v_dimension(const fsgpu_m2v *m); /* Embedder::dimension (crates/frankensearch-core/src/traits.rs:220-370) */
/* embed_batch_sync over token ids (model2vec_embedder.rs:310-335,409-419,435-451): text i owns
 * ids[offsets[i]..offsets[i+1]); out is [n,dim].  Empty / all-OOV texts give zeros. */
fsgpu_status fsgpu_m2v_embed(fsgpu_m2v *m, const uint32_t *ids, const uint32_t *offsets, uint32_t n, float *out);

/* ---- HashEmbedder: FNV-1a modular / JL projection from raw text, no weights ---- */
/* HashEmbedder::new (embed/src/hash_embedder.rs:215-223): the reference's test double and fast-tier fall-back (default_384 =
 * {384, FNV_MODULAR}, default_256 = {256, FNV_MODULAR}, jl_384(seed) = {384, JL_PROJECTION, seed}).  The vectors equal
 * embed_sync's in every bit: tokenize :601-685 (split on !char::is_alphanumeric, tokens of >= 2 UTF-8 bytes, case kept),
 * fnv1a_hash :588-595, embed_fnv_modular :263-280, embed_jl :299-346, l2_normalize_in_place (core/src/traits.rs:606-618).
 * alnum_bitmap_or_null: 0x110000 bits (139,264 bytes), bit c = byte[c >> 3] >> (c & 7) & 1 = char::is_alphanumeric of code point
 * c, made by the caller from its own toolchain's table and copied to the device once.  With NULL the embedder is ASCII only.
 * dimension 0 (the reference panics), dimension > 1,024 and an unknown algorithm are FSGPU_ERR_INVALID_CONFIG, decided before a
 * device is looked for; then no device is FSGPU_ERR_NO_DEVICE.  seed is read by FSGPU_HASH_JL_PROJECTION only. */
#define FSGPU_HASH_FNV_MODULAR 0   /* HashAlgorithm::FnvModular */
#define FSGPU_HASH_JL_PROJECTION 1 /* HashAlgorithm::JLProjection { seed } */
fsgpu_status fsgpu_hash_create(int32_t device, uint32_t dimension, int32_t algorithm, uint64_t seed,
                               const uint8_t *alnum_bitmap_or_null, fsgpu_hash **out);
void fsgpu_hash_destroy(fsgpu_hash *h);
uint32_t fsgpu_hash_dimension(const fsgpu_hash *h);
int32_t fsgpu_hash_device(const fsgpu_hash *h);
/* embed_batch_sync (:254-260): text i owns text_bytes[offsets[i]..offsets[i+1]); offsets must be non-decreasing and
 * text_bytes hold offsets[n] bytes; out is [n, dimension] f32; out_token_counts_or_null[n] = tokens hashed per text.  An empty or
 * token-less text gives zeros.  Refused with FSGPU_ERR_INVALID_CONFIG, *out_bad_text (nullable) = the first such text, nothing
 * written and nothing launched: a text with a byte >= 0x80 when the embedder has no table; with a table, a text that is not
 * strict UTF-8 (overlong forms, surrogates, values past U+10FFFF, truncated sequences: what a &str cannot hold); a text longer
 * than 32 MiB (it could hold 2^24 tokens, where the exact-integer argument of :294-298 ends).  Otherwise *out_bad_text is
 * 0xFFFFFFFF. */
fsgpu_status fsgpu_hash_embed(fsgpu_hash *h, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n, float *out,
                              uint32_t *out_token_counts_or_null, uint32_t *out_bad_text);
/* ... with the [n, dimension] output left in memory of the embedder's device, where
 * fsgpu_search_topk_batched_device_queries and fsgpu_index_builder_add_device take it. */
fsgpu_status fsgpu_hash_embed_device(fsgpu_hash *h, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n, float *out_dev,
                                     uint32_t *out_token_counts_or_null, uint32_t *out_bad_text);

/* ---- WordPiece tokenizer: raw text -> token ids on the device ---- */
/* The pipeline potion-base, all-MiniLM-L6-v2 and the ms-marco MiniLM cross-encoder ship in tokenizer.json: BertNormalizer ->
 * BertPreTokenizer -> WordPiece(continuing prefix, unk, max_input_chars_per_word) -> [CLS] ... [SEP].  The ids equal those of the
 * `tokenizers` crate for the same file, with no tolerance.  Everything that depends on Unicode tables or on the normalizer's
 * options (lowercase, strip_accents, handle_chinese_chars, clean_text) is the CALLER's table, made from the toolchain the caller
 * links; the device has no switch for any of them.
 *
 * cp_info[c] for input code point c (0 <= c < 0x110000):
 *   bits  0..20  FSGPU_WP_VALUE   len 1: the normalised code point; len 2..3: index of the first of `len` consecutive code
 *                                 points in `expansions`; len 0: ignored
 *   bits 21..23  FSGPU_WP_LEN     normalised length 0..3 (0 = the code point is dropped; above 3 is refused)
 *   bit  24      FSGPU_WP_SPACE   the (single) normalised code point separates words and belongs to none
 *   bit  25      FSGPU_WP_ISOLATE the (single) normalised code point is a word on its own (punctuation; a CJK character when the
 *                                 normalizer pads those with spaces)
 *   bit  26      FSGPU_WP_HOST    a text holding c cannot be tokenised here (see status below)
 *   bits 27..31  must be 0
 * SPACE and ISOLATE describe an entry of length 1; an entry of length 2..3 that would need either is given HOST by its maker.  An
 * entry whose `len` exceeds the UTF-8 length of c (1 for c < 0x80, 2 below 0x800, else 3) is treated as HOST: it keeps a text's
 * normalised length, and so its pieces, at or below its byte length.
 *
 * vocab_bytes / vocab_offsets[vocab_size + 1]: the tokens' UTF-8 bytes back to back, a token's id is its index.  prefix_bytes is
 * the continuing-subword prefix ("##", at most 16 bytes).  added_bytes / added_offsets[added_count + 1]: the contents of the added
 * tokens ("[CLS]", "[SEP]", "[PAD]", "[UNK]", "[MASK]", ...), at most 32 of 1..32 bytes each: `tokenizers` takes these out of the
 * raw text before it normalises, so a text that holds one is flagged, not tokenised.
 * FSGPU_ERR_INVALID_CONFIG, decided before a device is looked for: offsets that decrease (vocabulary or added tokens) or do not
 * start at 0, an empty vocabulary, unk_id / cls_id / sep_id >= vocab_size, two equal vocabulary entries, an expansion index out
 * of range, a length above 3, bits 27..31 set, a non-zero reserved word, max_input_chars_per_word 0 or above 1,024, a prefix over
 * 16 bytes, more than 32 added tokens, an added token of 0 or more than 32 bytes.  Then no device is FSGPU_ERR_NO_DEVICE. */
#define FSGPU_WP_CODE_POINTS 0x110000u
#define FSGPU_WP_VALUE_MASK 0x1FFFFFu
#define FSGPU_WP_LEN_SHIFT 21
#define FSGPU_WP_LEN_MASK 7u
#define FSGPU_WP_SPACE (1u << 24)
#define FSGPU_WP_ISOLATE (1u << 25)
#define FSGPU_WP_HOST (1u << 26)
typedef struct fsgpu_wordpiece_config {
    const uint8_t *vocab_bytes;
    const uint32_t *vocab_offsets; /* [vocab_size + 1] */
    uint32_t vocab_size;
    uint32_t unk_id, cls_id, sep_id;
    const uint8_t *prefix_bytes;
    uint32_t prefix_len;
    uint32_t max_input_chars_per_word; /* 100 in the three models' files */
    const uint32_t *cp_info;           /* [FSGPU_WP_CODE_POINTS] */
    const uint32_t *expansions;        /* [expansions_len] code points, may be NULL when expansions_len is 0 */
    uint32_t expansions_len;
    const uint8_t *added_bytes;
    const uint32_t *added_offsets;     /* [added_count + 1], may be NULL when added_count is 0 */
    uint32_t added_count;
    uint32_t reserved[8];              /* must be 0 */
} fsgpu_wordpiece_config;
fsgpu_status fsgpu_wordpiece_create(int32_t device, const fsgpu_wordpiece_config *config, fsgpu_wordpiece **out);
void fsgpu_wordpiece_destroy(fsgpu_wordpiece *tok);
int32_t fsgpu_wordpiece_device(const fsgpu_wordpiece *tok);
uint32_t fsgpu_wordpiece_vocab_size(const fsgpu_wordpiece *tok);
/* Tokenizer::encode_batch over single sequences, ids only.  Text i owns text_bytes[offsets[i]..offsets[i+1]), as in
 * fsgpu_hash_embed.  add_special_tokens != 0: [CLS] pieces [SEP].  max_length 0: no truncation; otherwise (truncation strategy
 * longest_first, direction right, stride 0) the first max_length - 2 * add_special pieces are kept; a max_length below the
 * special tokens' count is FSGPU_ERR_INVALID_CONFIG.  Output is a dense CSR: text i owns out_ids[out_offsets[i]..out_offsets[i+1]).
 *   out_status[i] 0: tokenised.  1: the text holds an added token's content or a HOST code point; it gets zero ids (no specials
 *     either), the other texts are unaffected and the call succeeds: such a text is the host tokenizer's.
 *   *out_total (nullable) = ids the batch needs.  ids_capacity below that: FSGPU_ERR_INVALID_CONFIG, *out_total set, nothing else
 *     written.
 *   Refused with FSGPU_ERR_INVALID_CONFIG, *out_bad_text (nullable) = the first such text, nothing launched and nothing written:
 *     a text that is not strict UTF-8 or is longer than 32 MiB; decreasing offsets are refused too.  Otherwise *out_bad_text is
 *     0xFFFFFFFF. */
fsgpu_status fsgpu_wordpiece_encode(fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n,
                                    int32_t add_special_tokens, uint32_t max_length, uint32_t *out_ids, uint64_t ids_capacity,
                                    uint32_t *out_offsets, uint8_t *out_status, uint64_t *out_total, uint32_t *out_bad_text);
/* ... with out_ids_dev [ids_capacity] and out_offsets_dev [n + 1] left in memory of the tokenizer's device (the shape
 * fsgpu_m2v_embed takes, without the trip); out_status and out_total stay on the host. */
fsgpu_status fsgpu_wordpiece_encode_device(fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets, uint32_t n,
                                           int32_t add_special_tokens, uint32_t max_length, uint32_t *out_ids_dev,
                                           uint64_t ids_capacity, uint32_t *out_offsets_dev, uint8_t *out_status,
                                           uint64_t *out_total, uint32_t *out_bad_text);
/* Tokenizer::encode_batch over pairs with special tokens: [CLS] a [SEP] (type 0) b [SEP] (type 1); out_type_ids parallels
 * out_ids.  max_length 0: no truncation; otherwise it is at least 3 and, with B = max_length - 3 and (la, lb) the pieces of a and
 * b, longest_first keeps: both when la + lb <= B; otherwise, with n1 <= n2 the two lengths sorted, n2 = n1 when n1 > B, else
 * max(n1, B - n1); when n1 + n2 still exceeds B, n1 = B / 2 and n2 = n1 + B % 2; the sort is then undone.  A pair is flagged
 * (status 1, zero ids) when either text is.  *out_bad_text names the pair whose a or b text is refused. */
fsgpu_status fsgpu_wordpiece_encode_pairs(fsgpu_wordpiece *tok, const uint8_t *a_bytes, const uint32_t *a_offsets,
                                          const uint8_t *b_bytes, const uint32_t *b_offsets, uint32_t n, uint32_t max_length,
                                          uint32_t *out_ids, uint32_t *out_type_ids, uint64_t ids_capacity, uint32_t *out_offsets,
                                          uint8_t *out_status, uint64_t *out_total, uint32_t *out_bad_text);
fsgpu_status fsgpu_wordpiece_encode_pairs_device(fsgpu_wordpiece *tok, const uint8_t *a_bytes, const uint32_t *a_offsets,
                                                 const uint8_t *b_bytes, const uint32_t *b_offsets, uint32_t n,
                                                 uint32_t max_length, uint32_t *out_ids_dev, uint32_t *out_type_ids_dev,
                                                 uint64_t ids_capacity, uint32_t *out_offsets_dev, uint8_t *out_status,
                                                 uint64_t *out_total, uint32_t *out_bad_text);
/* Model2VecEmbedder::embed_batch_sync from raw text (model2vec_embedder.rs:280-335: encode_fast(text, false), no special tokens,
 * no truncation): the texts are tokenised on the device and fsgpu_m2v_embed's kernel reads the ids where they lie; no id crosses
 * to the host.  tok and m must be on one device (else FSGPU_ERR_INVALID_CONFIG).  A flagged text is refused:
 * FSGPU_ERR_INVALID_CONFIG, *out_bad_text (nullable) = its index, the encoder is not run and out is not written. */
fsgpu_status fsgpu_m2v_embed_texts(fsgpu_m2v *m, fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets,
                                   uint32_t n, float *out, uint32_t *out_bad_text);
/* ... with the [n, dim] output left on the device. */
fsgpu_status fsgpu_m2v_embed_texts_device(fsgpu_m2v *m, fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets,
                                          uint32_t n, float *out_dev, uint32_t *out_bad_text);
/* NativeEmbedder::embed_batch_sync from raw text (native_embedder.rs:172-255): [CLS] pieces [SEP], truncated to max_length (0: not
 * truncated; a text then longer than the model's positions fails as in fsgpu_bert_embed), tokenised on the device; the forward
 * reads the ids where the tokenizer left them and gives the bits fsgpu_bert_embed gives for the same ids.  Only the n + 1 offsets
 * come back to the host, where the launches are planned.  tok and m on one device and the tokenizer's vocabulary no larger than the
 * model's, else FSGPU_ERR_INVALID_CONFIG.  A flagged text is refused as in fsgpu_m2v_embed_texts.  (Calls are not coalesced.) */
fsgpu_status fsgpu_bert_embed_texts(fsgpu_bert *m, fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets,
                                    uint32_t n, uint32_t max_length, float *out, uint32_t *out_bad_text);
fsgpu_status fsgpu_bert_embed_texts_device(fsgpu_bert *m, fsgpu_wordpiece *tok, const uint8_t *text_bytes, const uint32_t *offsets,
                                           uint32_t n, uint32_t max_length, float *out_dev, uint32_t *out_bad_text);
/* NativeReranker::rerank_sync's scoring from raw text (native.rs:1636-1710): pair i is [CLS] query [SEP] document i [SEP],
 * tokenised and truncated (longest_first to max_length, 0: not truncated) on the device as fsgpu_wordpiece_encode_pairs does; the
 * chain reads ids and type ids where the tokenizer left them and gives the logits and scores fsgpu_reranker_score gives for the
 * same pairs.  Document i owns doc_bytes[doc_offsets[i]..doc_offsets[i+1]).  A flagged query or document is refused:
 * FSGPU_ERR_INVALID_CONFIG, *out_bad_text (nullable) = the pair, nothing scored.  Device and vocabulary rules as above. */
fsgpu_status fsgpu_reranker_score_texts(fsgpu_reranker *m, fsgpu_wordpiece *tok, const uint8_t *query_bytes, uint32_t query_len,
                                        const uint8_t *doc_bytes, const uint32_t *doc_offsets, uint32_t n, uint32_t max_length,
                                        float *out_logits, float *out_scores, uint32_t *out_bad_text);

/* ---- MiniLM-class BERT embedder ---- */
/* NativeEmbedder::load (native_embedder.rs:60-116): copies the weights to the GPU (linears as f16). */
fsgpu_status fsgpu_bert_create(int32_t device, const fsgpu_bert_config *config, const fsgpu_bert_weights *weights,
                               fsgpu_bert **out);
/* The same from the model file itself — NativeEmbedder::load -> parse_weights (native.rs:1359-1602): `blob` is a safetensors file
 * (8-byte little-endian header length, JSON header, tensor bytes) in HuggingFace key layout.  F32 tensors only are read (I64
 * position_ids etc. are skipped); bare `embeddings.*` / `encoder.*` keys count as `bert.`-prefixed; pooler / classifier tensors
 * are ignored.  The model's shape comes from the tensors (vocab x hidden, layers by counting, inter, heads = hidden / 32, max_pos =
 * min(rows of the position table, 512)); ln_eps <= 0 means 1e-12.  A malformed blob / a missing or mis-shaped tensor is
 * FSGPU_ERR_MODEL_LOAD_FAILED with the reference's wording in fsgpu_last_error(); the blob is validated BEFORE a device is looked
 * for.  The tensor data must be 4-byte aligned in `blob` (it is when the file is read into a buffer malloc returned: the header
 * is padded to 8 bytes). */
fsgpu_status fsgpu_bert_create_safetensors(int32_t device, const void *blob, uint64_t blob_len, float ln_eps, fsgpu_bert **out);
/* Linear format, chosen at create time.  INT8_DYNAMIC is the arithmetic class of the reference's native forward
 * (native.rs:484-553,1506,1546-1600): every Linear weight int8 per output channel (quantised once at load), every Linear input int8
 * per row at forward, i32 accumulation, y = ((float)acc * (sx[m] * sw[n])) + b[n]; Q/K/V fused into one [3H, H] linear; embeddings,
 * LayerNorm, softmax, GELU and the residuals stay f32.  Quantisation of a row: amax = max |x|, inv = 127.0f / amax,
 * q = clamp(round_half_away(x * inv), -127, 127), scale = amax / 127.0f (all-zero row: q = 0, scale = 0).  It is NOT held to the f16
 * mode's tolerance against the f32 forward (cosine >= 0.995, max-abs <= 6e-2 instead of 0.999 / 2e-3), and a text's vector has the
 * same bits whatever batch it is embedded in.  hidden and inter must be multiples of 64 (they are of 128 for every model the
 * library takes). */
#define FSGPU_BERT_LINEAR_F16 0           /* default: f16 matrix-core linears (today's behaviour) */
#define FSGPU_BERT_LINEAR_INT8_DYNAMIC 1  /* native.rs: int8 per-output-channel weights, per-row dynamic int8 activations */
typedef struct fsgpu_bert_options {
    uint32_t linear_format;
    uint32_t reserved[7]; /* must be 0 */
} fsgpu_bert_options;
/* fsgpu_bert_create / fsgpu_bert_create_safetensors with options (NULL = FSGPU_BERT_LINEAR_F16, exactly the calls above).  An
 * unknown format or a non-zero reserved word is FSGPU_ERR_INVALID_CONFIG, reported before a blob is parsed or a device looked for. */
fsgpu_status fsgpu_bert_create_ex(int32_t device, const fsgpu_bert_config *config, const fsgpu_bert_weights *weights,
                                  const fsgpu_bert_options *options, fsgpu_bert **out);
fsgpu_status fsgpu_bert_create_safetensors_ex(int32_t device, const void *blob, uint64_t blob_len, float ln_eps,
                                              const fsgpu_bert_options *options, fsgpu_bert **out);
uint32_t fsgpu_bert_linear_format(const fsgpu_bert *m); /* FSGPU_BERT_LINEAR_*; 0 for NULL */
void fsgpu_bert_destroy(fsgpu_bert *m);
uint32_t fsgpu_bert_dimension(const fsgpu_bert *m); /* Embedder::dimension: the model's hidden size */
/* embed_batch_sync over token ids (native_embedder.rs:218-255 -> Model::embed_forward native.rs:1142-1236):
 * text i owns ids[offsets[i]..offsets[i+1]) (already tokenised WITH special tokens and truncated to <= 512,
 * no padding); every returned token is mean-pooled, then L2-normalised (zeros for empty / zero-norm,
 * fastembed_embedder.rs:416-426).  out is [n, hidden]. */
fsgpu_status fsgpu_bert_embed(fsgpu_bert *m, const int32_t *ids, const uint32_t *offsets, uint32_t n, float *out);

/* ---- MiniLM-class cross-encoder reranker ---- */
/* NativeReranker (native.rs:1240): a BertForSequenceClassification with num_labels = 1 over `[CLS] query [SEP] doc [SEP]` pairs —
 * typed embeddings, the encoder's layers (f16 matrix-core linears, as fsgpu_bert), the last layer for the [CLS] rows only
 * (encoder_layer_cls, native.rs:628-700), pooled = tanh(W_p cls + b_p), logit = w_c . pooled + b_c (forward_batch, :956-1130).
 * The encoder's shape rules are fsgpu_bert_create's; the reranker also needs hidden 128 / 256 / 384 (else FSGPU_ERR_INVALID_CONFIG).
 * A pair's logit has the same bits whatever call, batch, order or position it is scored in. */
typedef struct fsgpu_reranker_weights {
    fsgpu_bert_weights bert;     /* bert.type_emb holds type_vocab rows */
    uint32_t type_vocab;         /* token_type_embeddings rows (2 for BERT) */
    const float *pooler_w;       /* bert.pooler.dense.weight [H, H] */
    const float *pooler_b;       /* bert.pooler.dense.bias [H] */
    const float *classifier_w;   /* classifier.weight [1, H] */
    const float *classifier_b;   /* classifier.bias [1] */
} fsgpu_reranker_weights;
fsgpu_status fsgpu_reranker_create(int32_t device, const fsgpu_bert_config *config, const fsgpu_reranker_weights *weights,
                                   fsgpu_reranker **out);
/* The model file as a blob: fsgpu_bert_create_safetensors' rules (bare keys, F32 only, the blob checked before a device is looked
 * for), plus bert.pooler.dense.{weight,bias} and classifier.{weight,bias}, which are required; a classifier with more than one output
 * row is FSGPU_ERR_MODEL_LOAD_FAILED ("classifier: expected 1 logits, got N"). */
fsgpu_status fsgpu_reranker_create_safetensors(int32_t device, const void *blob, uint64_t blob_len, float ln_eps,
                                               fsgpu_reranker **out);
void fsgpu_reranker_destroy(fsgpu_reranker *m);
int32_t fsgpu_reranker_device(const fsgpu_reranker *m);
uint32_t fsgpu_reranker_max_length(const fsgpu_reranker *m); /* min(max_position_embeddings, 512); 0 for NULL */
/* Scores n pairs: pair i is ids[offsets[i]..offsets[i+1]) with type_ids alongside, already tokenised as [CLS] q [SEP] d [SEP] and
 * truncated by the caller (native.rs:1652-1666).  out_logits / out_scores [n]: score = sigmoid(logit) when the logit is finite, else
 * 0 (rerank_sync, native.rs:1631-1710).  An id >= vocab, a type id >= type_vocab or a pair longer than fsgpu_reranker_max_length is
 * FSGPU_ERR_INVALID_CONFIG, reported before anything runs; n = 0 is OK and does nothing; a zero-length pair gets logit 0 and score
 * 0.5 and changes nothing for the others.  Callers are served one at a time (native.rs:1668). */
fsgpu_status fsgpu_reranker_score(fsgpu_reranker *m, const int32_t *ids, const int32_t *type_ids, const uint32_t *offsets, uint32_t n,
                                  float *out_logits, float *out_scores);

/* ---- device-resident hand-offs: encoder -> search without the vectors crossing PCIe ---- */
/* The reference's seam between the two is a host Vec<f32> (traits.rs:401-582 -> search.rs:192); on the GPU both ends live in HBM.
 * fsgpu_bert_embed_device / fsgpu_m2v_embed_device are fsgpu_bert_embed / fsgpu_m2v_embed with the [n, dim] output left in device
 * memory `out_dev` (on the embedder's device; complete when the call returns).  It feeds fsgpu_search_topk_device /
 * fsgpu_search_topk_batched_device, fsgpu_search_topk_batched_device_queries (device queries, host results: what a serving loop
 * wants), or a sharded search through fsgpu_sharded_request::queries_dev.  fsgpu_device_malloc / _free give a host that links
 * nothing but this library the buffers for it. */
fsgpu_status fsgpu_bert_embed_device(fsgpu_bert *m, const int32_t *ids, const uint32_t *offsets, uint32_t n, float *out_dev);
fsgpu_status fsgpu_m2v_embed_device(fsgpu_m2v *m, const uint32_t *ids, const uint32_t *offsets, uint32_t n, float *out_dev);
fsgpu_status fsgpu_search_topk_batched_device_queries(fsgpu_index *idx, const float *queries_dev, uint32_t nq, uint32_t query_len,
                                                      uint32_t k, uint32_t *out_rows, float *out_scores, uint32_t *out_counts,
                                                      uint32_t *out_fallbacks);
/* fsgpu_search_topk_int8_two_pass_batched (search.rs:514-661 for a batch) with the queries already in device memory — the fast tier
 * of a many-queries two-tier flow takes the Model2Vec batch where fsgpu_m2v_embed_device left it (sync_searcher.rs:652-700 runs
 * embed -> search_fast_hits back to back; here neither the vectors nor a wait crosses PCIe in between). */
fsgpu_status fsgpu_search_topk_int8_two_pass_batched_device_queries(fsgpu_index *idx, const float *queries_dev, uint32_t nq,
                                                                    uint32_t query_len, uint32_t k, uint32_t candidate_multiplier,
                                                                    uint32_t *out_rows, float *out_scores, uint32_t *out_counts,
                                                                    uint32_t *out_fallbacks);
fsgpu_status fsgpu_device_malloc(int32_t device, uint64_t bytes, void **out);
fsgpu_status fsgpu_device_free(int32_t device, void *ptr);
int32_t fsgpu_bert_device(const fsgpu_bert *m);
int32_t fsgpu_m2v_device(const fsgpu_m2v *m);
int32_t fsgpu_index_device(const fsgpu_index *idx);

/* ---- device-resident hand-off: encoder -> index without the vectors crossing PCIe ---- */
/* VectorIndexWriter::write_record + finish (crates/frankensearch-index/src/lib.rs:3607-3672, 3752-3943), TwoTierIndexBuilder
 * (two_tier.rs:2003-2331), the facade's IndexBuilder (frankensearch/src/index_builder.rs:168-264) and RefreshWorker's rebuild
 * (fusion/src/refresh.rs) for vectors that sit in device memory: a builder takes (doc id, vector) batches from host memory, from
 * device memory or straight from an encoder handle, validates and encodes them on the device into a staging area, and at finish
 * leaves the sorted slab in device memory as a ready fsgpu_index, and the FSVI v1 file when a path is given.
 *
 * The contract is an equivalence.  After any sequence of successful adds, fsgpu_index_builder_finish(b, path, &idx, ...) leaves at
 * `path` the bytes fsgpu_fsvi_write_quant(path, embedder_id, embedder_revision, dim, n, all doc ids in arrival order, all vectors in
 * arrival order, compaction_gen, device, quantization) writes, and in `idx` a handle that behaves as fsgpu_index_open_fsvi(path,
 * device) of that file does: counts, doc ids, generation byte, slab bits, search rows and score bits, and later WAL appends, soft
 * deletes, compact and vacuum.  With path == NULL the handle is the same and no file is touched.  Zero records behave as
 * fsgpu_fsvi_write(n = 0) followed by fsgpu_index_open_fsvi.  The publication nonce is 0, as fsgpu_fsvi_write writes it.
 *
 * Validation (write_record_with_flags, lib.rs:3635-3673; vector_signal_usable, lib.rs:6133-6142) is per call and all-or-nothing, as
 * append_batch validates everything before anything changes.  vector_len != dim is FSGPU_ERR_DIMENSION_MISMATCH.  A row with a
 * non-finite element ("all embedding values must be finite"), a row whose norm_sq is not > 0 and finite ("embedding norm must be
 * non-zero and finite; a zero vector can never match any query": lib.rs:3658 in full, where fsgpu_fsvi_write stops at the
 * semicolon), a doc id longer than 65,535 bytes ("doc_id byte length must fit in u16"; an empty id is allowed) and, with
 * reject_duplicates, a doc id already staged or repeated inside the call ("duplicate doc_id; each document must have a unique id",
 * two_tier.rs:2125-2132) are FSGPU_ERR_INVALID_CONFIG.  The call then stages nothing, *out_bad_row (nullable) is the index in the
 * call of the first offending row, and the message is that row's first broken rule in the order above.  norm_sq is the
 * reference's: one f32 accumulator, the elements in order, a separate multiply and add, f32 subnormals kept; the check runs on the
 * device for host-memory adds too.  Values beyond the f16 range are legal and encode to +-inf, as f16::from_f32 encodes them.
 *
 * Staging grows in chunks of chunk_rows rows (nothing staged is ever copied to make room; an add refused for want of device memory,
 * FSGPU_ERR_DEVICE, stages nothing, keeps no allocation of its own and may be repeated with fewer rows); peak device memory at finish is the
 * staging + the final slab + the permutation (fsgpu_index_build_stats::peak_device_bytes).  The sort by (FNV-1a, doc id bytes)
 * stays on the host (lib.rs:3753-3762: stable, so duplicate ids keep their arrival order).  Calls on one builder are serialised
 * inside the library.  No device: FSGPU_ERR_NO_DEVICE; unknown option values or non-zero reserved words: FSGPU_ERR_INVALID_CONFIG
 * before a device is looked for. */
typedef struct fsgpu_index_builder fsgpu_index_builder;
typedef struct fsgpu_index_builder_options {
    uint32_t quantization;       /* 1 = F16 (default), 0 = F32 */
    uint32_t compaction_gen;     /* header byte, 0..255 */
    uint32_t reject_duplicates;  /* 0: VectorIndexWriter (duplicates kept, stable); 1: TwoTierIndexBuilder (two_tier.rs:2125-2132) */
    uint32_t chunk_rows;         /* staging chunk, 0 = library default (65,536 rows) */
    uint64_t reserve_rows;       /* hint: staging for this many rows is allocated at create; 0 = none */
    uint32_t reserved[6];        /* must be 0 */
} fsgpu_index_builder_options;
typedef struct fsgpu_index_build_stats {
    uint64_t rows, chunks;                      /* records in the index; staging chunks that were allocated */
    uint64_t ingest_launches, permute_launches; /* each covers at most 2^20 rows */
    double ingest_ms;                           /* all adds: first launch to verdict, host clock (uploads of host-memory adds included) */
    double sort_ms, permute_ms, tables_ms, file_ms;   /* finish: host sort, device gather, record + string tables, file (0 without a path) */
    double ingest_device_ms, permute_device_ms; /* the same two between events on the stream: the launches alone (and, for host-memory adds, the uploads between them) */
    uint64_t peak_device_bytes;                 /* staging + final slab + permutation + chunk table */
} fsgpu_index_build_stats;
/* options == NULL: {quantization 1, everything else 0}.  NULL embedder_id / embedder_revision are FSGPU_ERR_NULL_ARGUMENT. */
fsgpu_status fsgpu_index_builder_create(int32_t device, uint32_t dim, const char *embedder_id, const char *embedder_revision,
                                        const fsgpu_index_builder_options *options_or_null, fsgpu_index_builder **out);
void fsgpu_index_builder_destroy(fsgpu_index_builder *b);
uint64_t fsgpu_index_builder_record_count(const fsgpu_index_builder *b);   /* records staged so far; after finish: in the index */
/* doc_ids [n] pointers; doc_id_lens NULL = NUL-terminated ids.  vectors: [n, vector_len] f32 in host memory. */
fsgpu_status fsgpu_index_builder_add(fsgpu_index_builder *b, uint64_t n, const char *const *doc_ids, const uint32_t *doc_id_lens_or_null,
                                     const float *vectors, uint32_t vector_len, uint64_t *out_bad_row);
/* ... in memory of the builder's device.  The ingest is enqueued behind hip_stream (NULL = the default stream), the stream that
 * produced the vectors; the call returns when the verdict is known. */
fsgpu_status fsgpu_index_builder_add_device(fsgpu_index_builder *b, uint64_t n, const char *const *doc_ids,
                                            const uint32_t *doc_id_lens_or_null, const float *vectors_dev, uint32_t vector_len,
                                            void *hip_stream, uint64_t *out_bad_row);
/* ... embedded into a builder-owned device buffer by the very calls fsgpu_bert_embed_device / fsgpu_m2v_embed_device make, then
 * ingested.  An embedder on another device or of another dimension is FSGPU_ERR_INVALID_CONFIG / FSGPU_ERR_DIMENSION_MISMATCH; an
 * encoder error is returned as it is, with nothing staged.  An empty text embeds to zeros and is refused by the norm rule, naming
 * its row, as write_record would refuse it. */
fsgpu_status fsgpu_index_builder_add_bert(fsgpu_index_builder *b, fsgpu_bert *m, const int32_t *ids, const uint32_t *offsets, uint32_t n,
                                          const char *const *doc_ids, const uint32_t *doc_id_lens_or_null, uint64_t *out_bad_row);
fsgpu_status fsgpu_index_builder_add_m2v(fsgpu_index_builder *b, fsgpu_m2v *m, const uint32_t *ids, const uint32_t *offsets, uint32_t n,
                                         const char *const *doc_ids, const uint32_t *doc_id_lens_or_null, uint64_t *out_bad_row);
/* ... raw texts through a hash embedder, by the call fsgpu_hash_embed_device makes.  A text the embedder refuses is the call's
 * *out_bad_row; an empty or token-less text embeds to zeros and is refused by the norm rule naming its row, as above. */
fsgpu_status fsgpu_index_builder_add_hash(fsgpu_index_builder *b, fsgpu_hash *h, const uint8_t *text_bytes, const uint32_t *offsets,
                                          uint32_t n, const char *const *doc_ids, const uint32_t *doc_id_lens_or_null,
                                          uint64_t *out_bad_row);
/* VectorIndexWriter::finish (lib.rs:3752-3943).  The file, when path is given, is written to `path`.tmp and renamed over `path`, as
 * fsgpu_index_compact writes its image.  A finished builder is spent, as finish(self) consumes the reference's: only destroy and
 * record_count remain valid (anything else is FSGPU_ERR_INVALID_CONFIG).  A finish that fails (I/O, allocation) leaves the builder
 * whole and may be called again.  *out_index is the caller's to destroy. */
fsgpu_status fsgpu_index_builder_finish(fsgpu_index_builder *b, const char *path_or_null, fsgpu_index **out_index,
                                        fsgpu_index_build_stats *stats_or_null);

/* ---- host-side rank fusion (O(k), CPU, no GPU needed) ---- */
/* One ranked hit: ScoredResult / VectorHit as the fusion code reads them
 * (crates/frankensearch-core/src/types.rs:88-134): doc id (not NUL-terminated), score, vector row index. */
typedef struct fsgpu_scored_doc {
    const char *doc_id;
    uint32_t doc_id_len;
    float score;
    uint32_t index;
} fsgpu_scored_doc;
/* FusedHit (types.rs:3892-3925); ranks are -1 when absent, semantic_index 0xffffffff when absent;
 * doc_id points into the caller's input arrays. */
typedef struct fsgpu_fused_hit {
    const char *doc_id;
    uint32_t doc_id_len;
    double rrf_score;
    int64_t lexical_rank, semantic_rank;
    uint32_t semantic_index;
    float lexical_score, semantic_score;
    uint8_t in_both_sources;
} fsgpu_fused_hit;
#define FSGPU_RRF_TIEBREAK_LEXICAL_THEN_ID 0 /* RrfTiebreak::LexicalThenId (default, rrf.rs:52-66) */
#define FSGPU_RRF_TIEBREAK_HASH 1            /* RrfTiebreak::Hash */
/* rrf_fuse (crates/frankensearch-fusion/src/rrf.rs:368-560): score = sum over lanes of weight/(k+rank+1);
 * order (rrf desc, in_both desc, lexical score desc | doc-id hash, doc_id asc); window = offset..offset+limit.
 * Non-finite / negative k -> 60; non-finite / non-positive weights -> 1.  out holds `limit` entries. */
fsgpu_status fsgpu_rrf_fuse(const fsgpu_scored_doc *lexical, uint32_t n_lexical, const fsgpu_scored_doc *semantic,
                            uint32_t n_semantic, double k, double lexical_weight, double semantic_weight,
                            int32_t tiebreak, uint32_t limit, uint32_t offset, fsgpu_fused_hit *out,
                            uint32_t *out_count);
/* The rerank step after the model call (rerank_step_with_combine, crates/frankensearch-rerank/src/pipeline.rs:125-360).  candidates
 * [n] arrive in fused order and are reordered in place; rerank_score NaN = None; index is the caller's tag.  has_text[i] (NULL = all)
 * says whether candidate i has text; scores[n_scores] are the scores of the candidates WITH text inside the window
 * min(n, top_k_rerank), in window order.  Unchanged (out_applied = 0) when n < min_candidates, when fewer than min_candidates of the
 * window have text, or when n_scores is not that count.  Otherwise: the window's stale rerank scores are cleared, finite scores land
 * on their candidates, and the window is sorted — PURE_REORDER: rerank score desc (non-finite as -inf), doc_id bytes asc;
 * RRF_COMBINE: 1/(k + pre_rank) + 1/(k + rerank_rank) in f64 desc (ranks from 0, k = max(k, 1), a NaN k is 1), doc_id asc; a
 * window under 2 keeps its order.  Candidates past the window keep theirs.  Host only, O(window log window). */
typedef struct fsgpu_rerank_candidate {
    const char *doc_id;
    uint32_t doc_id_len;
    float score;          /* the fused score (carried along) */
    float rerank_score;   /* NaN = None */
    uint32_t index;
} fsgpu_rerank_candidate;
#define FSGPU_RERANK_PURE_REORDER 0 /* RerankCombine::PureReorder */
#define FSGPU_RERANK_RRF_COMBINE 1  /* RerankCombine::RrfCombine { k } */
fsgpu_status fsgpu_rerank_apply(fsgpu_rerank_candidate *candidates, uint32_t n, const uint8_t *has_text, const float *scores,
                                uint32_t n_scores, uint32_t top_k_rerank, uint32_t min_candidates, int32_t combine, float k,
                                uint8_t *out_applied);
/* blend_two_tier (crates/frankensearch-fusion/src/blend.rs:107-195): per-list min-max normalisation,
 * alpha*quality + (1-alpha)*fast (single-source docs keep their normalised score), order (score desc, doc_id asc).
 * out holds n_fast + n_quality entries. */
fsgpu_status fsgpu_blend_two_tier(const fsgpu_scored_doc *fast, uint32_t n_fast, const fsgpu_scored_doc *quality,
                                  uint32_t n_quality, float blend_factor, fsgpu_scored_doc *out, uint32_t *out_count);
/* blend_two_tier_aligned (blend.rs:213-294; the vector-index specialisation :296-358 gives the same output for unique doc ids):
 * the quality tier as per-position scores of the SAME hits — quality_scores[i] belongs to fast[i] and counts only where
 * quality_present[i] != 0 (the Option<f32> of quality_scores_for_hits).  Fast bounds over all fast scores, quality bounds over
 * the present scores, first occurrence of a doc id wins both slots.  out holds n_fast entries. */
fsgpu_status fsgpu_blend_two_tier_aligned(const fsgpu_scored_doc *fast, uint32_t n_fast, const float *quality_scores,
                                          const uint8_t *quality_present, float blend_factor, fsgpu_scored_doc *out,
                                          uint32_t *out_count);

/* ---- TwoTierIndex: the pairing of a fast and a quality index (crates/frankensearch-index/src/two_tier.rs) ---- */
/* QualityAlignment (two_tier.rs:404-409), computed once when the pair is opened (two_tier.rs:750-866): both record tables are
 * sorted by (FNV-1a(doc_id), doc_id), so one merge pass — tombstoned rows skipped on either side — maps every fast row to its
 * quality row; the result stays ALIGNED (fast row i = quality row i) until the first divergence and becomes a per-row MAPPING
 * after it.  Raw slabs (no record table) pair by row.  The indexes stay owned by the caller and must outlive the alignment;
 * rebuild it after a tombstone update of either index (the reference computes it at open). */
typedef struct fsgpu_alignment fsgpu_alignment;
#define FSGPU_ALIGNMENT_NONE 0
#define FSGPU_ALIGNMENT_ALIGNED 1
#define FSGPU_ALIGNMENT_MAPPING 2
fsgpu_status fsgpu_alignment_create(fsgpu_index *fast, fsgpu_index *quality, fsgpu_alignment **out);
void fsgpu_alignment_destroy(fsgpu_alignment *a);
int32_t fsgpu_alignment_kind(const fsgpu_alignment *a);
/* quality_index_for_fast_index (two_tier.rs:1975-1981): -1 when the fast row has no quality row */
int64_t fsgpu_alignment_quality_row(const fsgpu_alignment *a, uint64_t fast_row);
uint64_t fsgpu_alignment_unmatched_quality_docs(const fsgpu_alignment *a);
/* TwoTierIndex::quality_scores_for_hits (two_tier.rs:1566-1631): the phase-2 scoring of an UNATTESTED quality tier — every
 * FSVI v1 artifact (sync_searcher.rs:810-818).  Per fast hit: the quality WAL's latest resident entry of the doc id
 * (dot_product_f32_f32 on the host), else the aligned quality row (hit.index == 0xffffffff looks the fast row up by doc id
 * first), else the quality index's own live row of that doc id; main rows are scored by ONE gather launch of
 * dot_product_f16_bytes_f32 in the scan's operation order (dot_query_at).  out_present[i] == 0 is the reference's None.
 * hits[i].doc_id may be null for raw-slab pairs.  FSGPU_ERR_DIMENSION_MISMATCH when query_len is not the quality dimension. */
fsgpu_status fsgpu_quality_scores_for_hits(fsgpu_index *fast, fsgpu_index *quality, const fsgpu_alignment *alignment,
                                           const float *query, uint32_t query_len, const fsgpu_scored_doc *hits, uint32_t n,
                                           float *out_scores, uint8_t *out_present);
/* quality_scores_for_hits for a CHUNK of queries (the many-queries two-tier flow, fshost_two_tier_search_many with
 * FSHOST_POOL_RESCORED): query q owns hits[hit_offsets[q] .. hit_offsets[q + 1]) and queries[q * query_len ..); every hit is
 * resolved as above (two_tier.rs:1566-1631), and the dots over the quality tier's main rows of ALL the queries run as ONE gather
 * launch.  out_scores / out_present are aligned with `hits`.  Same scores, bit for bit, as nq calls of the function above. */
fsgpu_status fsgpu_quality_scores_for_hits_batched(fsgpu_index *fast, fsgpu_index *quality, const fsgpu_alignment *alignment,
                                                   const float *queries, uint32_t nq, uint32_t query_len,
                                                   const fsgpu_scored_doc *hits, const uint32_t *hit_offsets, float *out_scores,
                                                   uint8_t *out_present);

/* TwoTierIndex over two row-sharded handles (fast and quality slabs shard identically).  The alignment walk reads the
 * handles' catalogs (fsgpu_sharded_open_fsvi; raw shards pair by row); quality_scores_for_hits resolves WAL entries and doc ids
 * there and gathers dot_query_at on the shards that own the quality rows (one gather launch per shard touched).  Same outputs
 * as fsgpu_quality_scores_for_hits over unsharded indexes with the same rows. */
fsgpu_status fsgpu_sharded_alignment_create(fsgpu_sharded *fast, fsgpu_sharded *quality, fsgpu_alignment **out);
fsgpu_status fsgpu_sharded_quality_scores_for_hits(fsgpu_sharded *fast, fsgpu_sharded *quality, const fsgpu_alignment *alignment,
                                                   const float *query, uint32_t query_len, const fsgpu_scored_doc *hits, uint32_t n,
                                                   float *out_scores, uint8_t *out_present);

/* ---- MMR: diversified reranking over document vectors ---- */
/* Maximum Marginal Relevance exactly as the reference states it (crates/frankensearch-fusion/src/mmr.rs:103-319; the stage after
 * the rerank step in TwoTierSearcher, searcher.rs:2696-2745).  All arithmetic is f64: n = min(len, candidate_pool), k = min(k, n);
 * relevance is min-max normalised over the pool's finite scores (non-finite -> 0, a range below f64::EPSILON -> 1); sim(i, j) is
 * cosine_sim_pre — four accumulators, element e to acc[e % 4], ((a0 + a1) + a2) + a3, the tail in order, divided by the product of
 * the root norms (one sequential accumulator each), 0 when that product is below f64::EPSILON —, or cosine_sim (one accumulator
 * each) when the pool's vectors differ in length; the first pick is the first greatest relevance, then greedy rounds of
 * fma(lambda, relevance, -((1 - lambda) * max sim to the selected)) with a strict `>` (lowest index wins a tie), ending early when
 * no candidate beats -inf.  The order is a list of indexes into the pool.
 * MmrConfig (mmr.rs:43-66): defaults enabled = 0, lambda = 0.7, candidate_pool = 30 (fsgpu_mmr_config_default).  lambda is clamped
 * (non-finite or negative -> 0, above 1 -> 1).  enabled must be 0 or 1 and the reserved words 0, else FSGPU_ERR_INVALID_CONFIG.
 * A NULL config means the defaults. */
typedef struct fsgpu_mmr_config {
    uint32_t enabled;
    uint32_t candidate_pool;
    double lambda;
    uint32_t reserved[4]; /* must be 0 */
} fsgpu_mmr_config;
fsgpu_status fsgpu_mmr_config_default(fsgpu_mmr_config *config);
/* mmr_rerank on caller-supplied f32 vectors (vectors[i] holds lengths[i] values; ragged pools allowed), on the host: no device is
 * needed.  out_order holds min(k, n, candidate_pool) entries, *out_count says how many were selected; out_sims (may be NULL) receives
 * the pool x pool matrix of sim(i, j), pool = min(n, candidate_pool).  This is also what the index-level calls below run for a
 * pool the kernel does not take, with the same bits. */
fsgpu_status fsgpu_mmr_rerank(const double *scores, const float *const *vectors, const uint32_t *lengths, uint32_t n, uint32_t k,
                              double lambda, uint32_t candidate_pool, uint32_t *out_order, uint32_t *out_count, double *out_sims);
/* VectorIndex::vector_at_f32 (crates/frankensearch-index/src/lib.rs:3142): row `row` of the slab widened to f32; out holds
 * dimension values.  An out-of-range row is FSGPU_ERR_INVALID_CONFIG. */
fsgpu_status fsgpu_index_vector_at_f32(fsgpu_index *idx, uint32_t row, float *out);
/* mmr_rerank over rows of one index, on its device (mmr_kernels.hip: one workgroup per pool; the rows are gathered from the slab
 * where they are, only scores go up and indexes come back).  rows[n] are global row ids, scores[n] their relevance; config's
 * lambda and candidate_pool apply (enabled is not consulted: as mmr_rerank itself, the caller decides whether to call).  out_order
 * holds n entries of which the first *out_count are written.  out_sims (may be NULL) receives the pool x pool similarity matrix.
 * The batched form takes nq pools — pool q owns rows / scores / out_order [offsets[q], offsets[q + 1]) — in ONE launch; a pool's
 * order is the same whatever batch it rides in.  Pools of up to 128 rows at up to 384 dimensions and up to 64 rows at up to 1,024
 * (rows * dimension <= 65,536) run on the device; a larger pool runs fsgpu_mmr_rerank on vectors fetched from the slab, with the
 * same bits.  A row out of range is FSGPU_ERR_INVALID_CONFIG.  Row-sharded handles (fsgpu_sharded) have no MMR call: a pool's rows
 * sit on several GPUs. */
fsgpu_status fsgpu_index_mmr_rerank(fsgpu_index *idx, const uint32_t *rows, const double *scores, uint32_t n, uint32_t k,
                                    const fsgpu_mmr_config *config, uint32_t *out_order, uint32_t *out_count, double *out_sims);
fsgpu_status fsgpu_index_mmr_rerank_batched(fsgpu_index *idx, const uint32_t *rows, const double *scores, const uint32_t *offsets,
                                            uint32_t nq, uint32_t k, const fsgpu_mmr_config *config, uint32_t *out_order,
                                            uint32_t *out_counts);
/* The searcher's MMR stage over one index (searcher.rs:2696-2745).  docs[n] is the result list in rank order (doc id and f32 score;
 * index is not read).  Nothing happens (identity order, *out_applied = 0) when config is not enabled, n < 2 or the pool
 * min(n, max(candidate_pool, 1)) is below 2.  Each document of the pool resolves as quality_vector_for_doc_id does within one index
 * (two_tier.rs:1857-1872): its newest WAL entry, else the first live main row with that id; a document that resolves to nothing
 * leaves the list untouched (identity, *out_applied = 0), and so does a selection shorter than the pool.  Otherwise out_order[n] is
 * the MMR order of the pool (k = pool, scores widened to f64) followed by the tail in place, and *out_applied = 1.  WAL vectors
 * travel to the kernel as per-candidate overrides.  The index needs a doc-id table. */
fsgpu_status fsgpu_index_mmr_rerank_docs(fsgpu_index *idx, const fsgpu_scored_doc *docs, uint32_t n, const fsgpu_mmr_config *config,
                                         uint32_t *out_order, uint8_t *out_applied);
/* The same stage over a fast / quality pair (semantic_vector_with_tier_for_doc_id, two_tier.rs:1832-1925): per document the
 * quality tier first — the quality WAL's newest entry, the aligned quality row of its live fast row, the quality index's own row —
 * then the fast tier (its WAL, its live row).  Raw slabs without doc-id tables resolve hits[i].index as the fast row.  When every
 * vector comes from one tier the pool runs on that tier's device; a pool that mixes tiers is fetched (fsgpu_index_vector_at_f32)
 * and runs fsgpu_mmr_rerank, ragged if the tiers' dimensions differ.  Outputs as fsgpu_index_mmr_rerank_docs. */
fsgpu_status fsgpu_two_tier_mmr_rerank(fsgpu_index *fast, fsgpu_index *quality, const fsgpu_alignment *alignment,
                                       const fsgpu_scored_doc *hits, uint32_t n, const fsgpu_mmr_config *config, uint32_t *out_order,
                                       uint8_t *out_applied);

/* ---- query hubness: the r_d table and the phase-1 penalty ---- */
/* The reference's query-hubness correction (crates/frankensearch-fusion/src/hubness.rs; applied by TwoTierSearcher's
 * correct_phase1_pool, searcher.rs:737-777, 1869-1873).  r_d is the mean of document d's k = min(kq, n_queries) greatest
 * similarities to a background query sample; the penalty is s' = s - beta * r_d over the fast-tier pool, then one re-sort.
 *   sim(d, j) = dot_product_f32_f32 (crates/frankensearch-index/src/simd.rs:134-222) in the horizontal order `hreduce`: four 8-lane
 *     accumulators over groups of 32 with a separate multiply and add, (acc0 + acc1) + (acc2 + acc3), the leftover 8-element chunks
 *     added to that sum AFTER the tree, reduce_add, then the last n % 8 elements as an unfused multiply and add.  (The scan's f16
 *     byte dot puts the leftovers into acc0 before the tree and fuses its tail; the F32-slab byte dot fuses its tail.)
 *   selection: the k greatest under f32::total_cmp (hubness.rs:135): -0.0 < +0.0, +NaN above +inf, -NaN below -inf.
 *   mean: the reference sums `top` in whatever order select_nth_unstable_by left it, which pins the multiset but not the bits.
 *     This library fixes ONE of those orders, on every path: v_1 >= ... >= v_k; s = v_1; s += v_2; ...; s += v_{k-1};
 *     r_d = (v_k + s) / (float)k; for k == 1, v_1 / 1.0f.
 *   an empty sample or kq == 0 gives zeros; every row gets an entry, tombstoned rows too (the table is indexed by VectorHit::index).
 * HubnessConfig (hubness.rs:36-58): defaults beta = 0.2, kq = 10; the reserved words must be 0. */
typedef struct fsgpu_hubness_config {
    float beta;
    uint32_t kq;
    uint32_t reserved[4]; /* must be 0 */
} fsgpu_hubness_config;
fsgpu_status fsgpu_hubness_config_default(fsgpu_hubness_config *config);
/* compute_query_hubness on caller-supplied f32 vectors, on the host (no device is needed): docs[d] holds doc_lens[d] values,
 * queries[j] query_lens[j]; each dot runs over the common prefix of its two vectors, as the reference's does (hubness.rs:157-161).
 * out[n_docs].  Threaded over rows (OMP_NUM_THREADS threads, at most 16); a row's value does not depend on the thread count or on
 * the other rows.  This is also what the index-level calls below run for k > 64, with the same bits. */
fsgpu_status fsgpu_query_hubness(const float *const *docs, const uint32_t *doc_lens, uint64_t n_docs, const float *const *queries,
                                 const uint32_t *query_lens, uint32_t n_queries, uint32_t kq, int32_t hreduce, float *out);
/* apply_hubness_penalty (hubness.rs:67-86) in place: the identity (*out_applied = 0) when beta is non-finite or <= 0; otherwise
 * score - beta * r as a separate f32 multiply and subtract with r = table[index], or 0 when index >= table_len.  resort != 0 then
 * sorts as correct_phase1_pool does, by VectorHit::cmp_rank (types.rs:101-133): score descending with NaN as -inf, doc_id bytes
 * ascending.  A NULL config means the defaults. */
fsgpu_status fsgpu_apply_hubness_penalty(fsgpu_scored_doc *hits, uint32_t n, const float *table, uint64_t table_len,
                                         const fsgpu_hubness_config *config, int32_t resort, uint8_t *out_applied);
/* compute_query_hubness over every row of an index, on its device (hubness_kernels.hip): a workgroup keeps a tile of rows in LDS
 * widened to f32 (exact for an f16 slab), streams the query sample past it and keeps a running top-k per row; the slab is read
 * once.  queries[nq, query_dim] are host values, out[record_count] is written in row order, the call blocks.  It runs on the
 * index's own stream with workspaces of its own.  query_dim must equal the index's dimension (FSGPU_ERR_DIMENSION_MISMATCH): this
 * is STRICTER than the reference, whose dot truncates to the common length — use fsgpu_query_hubness for ragged inputs.
 * k = min(kq, nq) <= 64 at up to 1,024 dimensions runs on the device; anything else runs fsgpu_query_hubness over rows fetched
 * from the slab in blocks, with the same bits — on the HOST, tens of seconds at corpus size, and like every call on an index it
 * holds the index for its whole duration: searches on the same handle wait behind it.  Build such a table on a handle that is not
 * serving, or keep kq <= 64.  (A similarity that is a NaN GENERATED by the arithmetic — inf - inf, 0 x inf —
 * has an architecture-defined sign; such rows are outside the bit contract between the two.)  Without a device:
 * FSGPU_ERR_NO_DEVICE. */
fsgpu_status fsgpu_index_compute_query_hubness(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                               float *out);
/* The same over a row-sharded handle: every row shard computes its own rows, the results are concatenated in global row order.  No
 * collective: a row's value does not depend on the layout. */
fsgpu_status fsgpu_sharded_compute_query_hubness(fsgpu_sharded *sh, const float *queries, uint32_t nq, uint32_t query_dim, uint32_t kq,
                                                 float *out);

/* ---- the k-NN graph over the main slab and the phase-1 neighbour smoothing ---- */
/* The reference's k-NN graph diffusion (crates/frankensearch-fusion/src/smooth.rs; second step of correct_phase1_pool,
 * searcher.rs:737-777) walks the `Similar` edges of a DocumentGraph, "nearest-first, as a k-NN builder produces" (smooth.rs:126-129);
 * the reference has no such builder.  This is one, exact, on the device.
 * THE GRAPH IS DEFINED BY THE INDEX'S OWN SEARCH.  For a main row i, knn(i, m) is the first m live main rows j != i under the
 * reference's total order — key(score) descending with NaN as -inf, row ascending — where score(i, j) is what a row-level exact
 * search of this index returns for the query q = row i widened to f32 (exact for an F16 slab; an F32 slab uses its own values):
 * dot_product_f16_bytes_f32 / dot_product_f32_bytes_f32 in the index's current hreduce order.  Equivalently: take the row-level
 * top-(m + 1) of that query, remove the entry whose row is i if it is there, otherwise drop the last entry (which happens when more
 * than m lower-numbered duplicates of row i exist).
 *   - tombstoned rows are never targets; as sources they get an empty list.  No search is run for them.
 *   - resident WAL entries take no part: the graph is over the main slab.  There is no doc-id dedup.
 *   - a list shorter than m (fewer than m + 1 live rows, a tombstoned source) is padded with 0xffffffff rows and 0.0f similarities.
 *   - row ids are global: row_base is added, as in every search.
 * The call covers the sources first_row .. first_row + n_rows: out_rows [n_rows, m] u32 and out_sims [n_rows, m] f32 (may be NULL)
 * are HOST arrays, list r at offset (r - first_row) * m; the call blocks.  1 <= m <= 63, so that k = m + 1 stays inside the fused
 * tiers of the batched search; anything else, or a range past record_count, is FSGPU_ERR_INVALID_CONFIG.  n_rows == 0 is OK and does
 * nothing.  Without a device: FSGPU_ERR_NO_DEVICE.  Errors are reported before any work starts.
 * HOW IT RUNS.  No second scan: the live sources are staged from the slab, up to 1,024 per step, into an f32 query block in HBM
 * (knn_stage_rows_kernel), answered by the batched search unchanged — int8 filter under its proven bound, finish in the reference's
 * order, fallbacks as they are (fsgpu_search_topk_batched_device_begin / _end_late) — and turned into lists by knn_emit_kernel, which
 * finds the self entry with a ballot and shifts the tail up.  Rows, queries and hits stay in HBM; the lists come up through a pinned
 * block, one copy per step, underneath the next step's search.  Two steps are in flight: the call uses BOTH search tickets of the
 * handle and holds the index for its whole duration, so searches on the same handle wait behind it, and it is refused
 * (FSGPU_ERR_INVALID_CONFIG) while a begun search is outstanding.  The range arguments let a caller build in slices between
 * searches and resume a partial build; slices concatenate to the whole-graph call.  Which path answers the searches is the batched
 * search's own choice (slabs under 32,768 rows, F32 slabs and dimensions outside 64 / 128 / 256 / 384 take the exact kernels): the
 * graph is the same by definition on every path. */
fsgpu_status fsgpu_index_build_knn_graph(fsgpu_index *idx, uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t *out_rows,
                                         float *out_sims);
/* The same over a row-sharded handle: every row shard's live rows are the queries of sharded batched searches over ALL shards, in
 * global row order; the result equals the unsharded graph over the same rows for every layout.  The sources are STAGED THROUGH THE
 * HOST here: the owning shard widens a step's rows to f32 and copies them up ([1,024, dim] f32, 1.5 MB at 384 dimensions), the
 * sharded search sends them to every shard like any host batch, and the self rule runs on the host over the merged hits — one
 * round trip of the query block per step beside a scan of every shard's slab, overlapped with the step before (two tickets).  The
 * sharded search's own limits apply (dimension a multiple of 8). */
fsgpu_status fsgpu_sharded_build_knn_graph(fsgpu_sharded *sh, uint64_t first_row, uint64_t n_rows, uint32_t m, uint32_t *out_rows,
                                           float *out_sims);
/* ---- carrying the k-NN graph across a compaction, a vacuum or deletes ----
 * The table is the most expensive object derived from an index and a rewrite renumbers its rows, yet nearly all of it survives: a
 * compaction with W WAL entries changes the lists of the W new rows, of the sources that listed a dropped row, and of the sources for
 * which a new row now beats their m-th neighbour.  Every other list is the old list with its ids renumbered.
 * INPUTS.  The index as it is now (slab, live bitmap, row_base, hreduce order); m, 1 <= m <= 63; an old table old_rows [old_len, m]
 * u32 and old_sims [old_len, m] f32, BOTH required, global ids relative to old_row_base with 0xffffffff / 0.0f padding; a map
 * new_to_old [record_count] u32: entry x is the old LOCAL row that current row x is a byte-for-byte copy of, or 0xffffffff when x has
 * no predecessor.  NULL means the identity with old_len == record_count: nothing was renumbered, only the live bitmap changed.
 * GUARANTEE.  If old_rows / old_sims are what fsgpu_index_build_knn_graph(.., 0, old_len, m, ..) returned on an index in some state
 * E0, new_to_old says truthfully which current rows are copies of which E0 rows, and the hreduce order is the same, then out_rows /
 * out_sims [record_count, m] equal BYTE FOR BYTE what fsgpu_index_build_knn_graph(idx, 0, record_count, m, ..) returns on the
 * current index.  The old table may come from another handle (an index since closed).  For inputs that break the premise the result
 * is unspecified but memory-safe: every id of the table and the map is range-checked before it becomes an address.
 * CLASSES of a current row x, a pure function of the inputs:
 *   - dead: x is not live now.  Its list is all padding and it is nobody's target.
 *   - added: x is live and has no predecessor, or its predecessor's old list is empty (column 0 is the pad: a row that was
 *     tombstoned when the table was built and is live again, or a row of an index that then had one live row).  It gets a full search
 *     and is a candidate for every other list.
 *   - kept: x is live and its predecessor has a non-empty list.  Each old entry before the list's first pad is mapped global id ->
 *     old local row -> current row (the inverse of new_to_old); it is DROPPED if its id lies outside [old_row_base, old_row_base +
 *     old_len), it has no current row, or its current row is dead now.
 *       kept-dirty: an entry is dropped.  The list lost a neighbour whose replacement is unknown: a full search.
 *       kept-clean: otherwise.  The list is the first m under the total order of (the mapped old entries with their OLD sims) u
 *       (the added rows a with score(x, a)), as global ids, then padding.
 *   - monotonicity: that a kept-clean list is still the top-m over the kept rows needs ties to break as before, so the predecessors
 *     must increase with x over the rows that have one (a compaction or a vacuum of a sorted record table guarantees it).  If they
 *     do not, every kept row is dirty: a full rebuild inside the call, still exact, stats.rebuilt = 1.
 * score(x, a) comes from a transposed exact join (knn_update_join_kernel): x widened to f32 in LDS, the added rows streamed past.
 * Each product f32(x_e) * f32(a_e) commutes and the byte dots' accumulation order depends on the element index alone, so the join
 * reproduces dot_product_f16_bytes_f32 / dot_product_f32_bytes_f32 bit for bit (leftover chunks into accumulator 0 before the tree
 * for F16, after the tree for F32; a fused tail) in all three hreduce orders.
 * FALLING BACK TO A REBUILD, the same table either way, every live row searched inside the call: rebuilt = 1 the map is not
 * monotone; 2 added > max_added_fraction * record_count (compared in f64; the default is fsgpu_knn_update_config_default's); 3 a
 * shape the join does not cover (dimension above 1,024, an MRL prefix view).  When several hold the first of 1, 3, 2 is reported.
 * REFUSALS, FSGPU_ERR_INVALID_CONFIG before any work and with nothing written: m outside 1 .. 63; NULL tables or outputs; old_len >=
 * 2^32 - 1; a new_to_old entry that is neither 0xffffffff nor < old_len; two current rows naming the same predecessor; identity mode
 * with old_len != record_count; non-zero reserved words; a begun search outstanding (the call holds the index exactly as the graph
 * build does and takes both tickets).  No device: FSGPU_ERR_NO_DEVICE.  An empty index: OK, nothing done.  out_* must not alias
 * old_*.  All arrays are HOST arrays; the call blocks.  Sharded handles are not covered. */
typedef struct fsgpu_knn_update_config {
    float max_added_fraction;
    uint32_t reserved[7]; /* must be 0 */
} fsgpu_knn_update_config;
fsgpu_status fsgpu_knn_update_config_default(fsgpu_knn_update_config *config);
typedef struct fsgpu_knn_update_stats {
    uint64_t rows, dead, added, kept_clean, kept_dirty;
    uint64_t searched_sources; /* sources answered by the batched search: added + kept_dirty, or every live row when rebuilt */
    uint64_t join_pairs;       /* kept_clean x added, 0 when rebuilt */
    uint64_t join_entries;     /* entries of the OUTPUT's kept-clean lists that are added rows */
    uint32_t rebuilt;          /* 0 incremental; 1 map not monotone; 2 added > max_added_fraction * rows; 3 a shape the join does not cover */
    uint32_t reserved;
    double device_ms, join_ms;
} fsgpu_knn_update_stats;
fsgpu_status fsgpu_index_update_knn_graph(fsgpu_index *idx, uint32_t m, const uint32_t *old_rows, const float *old_sims, uint64_t old_len,
                                          uint32_t old_row_base, const uint32_t *new_to_old_or_null,
                                          const fsgpu_knn_update_config *config_or_null, uint32_t *out_rows, float *out_sims,
                                          fsgpu_knn_update_stats *stats_or_null);
/* new row -> the main row of the index BEFORE the last compaction / vacuum that changed the slab it is a copy of, 0xffffffff for a
 * row that came from the WAL.  out [record_count]; generation_before / _after (may be NULL) are fsgpu_index_generation on both sides;
 * old_record_count (may be NULL) is the row count before.  The handle keeps the rewrite's runs, not 4 bytes per row.
 * FSGPU_ERR_INVALID_CONFIG when no rewrite has happened on this handle.  Maps of several rewrites are not composed: update after
 * each rewrite, or compose them. */
fsgpu_status fsgpu_index_rewrite_sources(fsgpu_index *idx, uint32_t *out_new_to_old, uint64_t *generation_before, uint64_t *generation_after,
                                         uint64_t *old_record_count);
/* The graph optimisation: a neighbour table in, a navigable table of lower degree out.  An exact k-NN table is a poor
 * graph to search: its lists are redundant (a row's nearest neighbours are mostly each other's neighbours), no edge leaves a tight
 * group, and rows that nobody lists cannot be reached.  The repair is CAGRA's graph optimisation, restated as a PURE FUNCTION of the
 * table: it reads no vector, computes no distance and does not look at the live bitmap (rows deleted after the build stay in the
 * lists; the search tests the bitmap when it runs), so the result is the same bytes on every run and every device.
 * Inputs: T [N, w] global u32 ids with 0xffffffff as the pad, the index's row_base, N = record_count, an output degree d,
 * 1 <= d <= w <= 64.  Output: [N, d].
 *   1. clean list C(x): walk T[x] from column 0 to the first pad; keep a global id g if r = g - row_base lies in [0, N), r != x and
 *      r was not kept before.  Rank i is the position in C(x).  The table is the caller's: every id is checked against N before it
 *      becomes an address.
 *   2. detour count: for rank i with y = C(x)[i], cnt[i] is the number of ranks j < i such that, in the raw list of z = C(x)[j]
 *      (the columns of T[z] before its first pad), y's global id first occurs at a column p < i.  The route x -> z -> y detours the
 *      edge x -> y when both of its hops rank above it.
 *   3. forward list F(x): the ranks sorted by (cnt ascending, i ascending), the first d of them.
 *   4. reverse candidates of y: all pairs (r, x) with F(x)[r] = y, ordered by (r ascending, x ascending); only the first d matter.
 *      No arrival order of any atomic reaches the result.
 *   5. output list of x, h = ceil(d / 2): the first h entries of F(x); then the reverse candidates of x in order, skipping rows
 *      already present, until d entries; then the rest of F(x) in order, skipping rows already present, until d entries.  Written as
 *      global ids, dense from column 0, then pads: no pad stands before an entry.
 * graph_rows [graph_len, graph_width] and out_rows [graph_len, out_degree] are HOST arrays (fsgpu_index_build_knn_graph's output,
 * fsgpu_ann_create's input); the index supplies the device, the stream and row_base; the call blocks, and its workspace comes and goes
 * with it.  Refused with FSGPU_ERR_INVALID_CONFIG before any work and with nothing written: graph_len != record_count, out_degree 0
 * or above graph_width, graph_width above 64, a NULL table or output.  Without a device: FSGPU_ERR_NO_DEVICE.  An empty index returns
 * OK and does nothing.  The call holds the index the way the k-NN build does and is refused (FSGPU_ERR_INVALID_CONFIG) while a begun
 * search is outstanding.
 * stats (may be NULL): forward_edges / reverse_edges count the output's entries by origin (F, reverse candidates);
 * zero_in_degree_before / _after count the rows no edge points at in the first out_degree columns of the input, walked as the search
 * walks them (to the first pad; an id outside the table or the row itself is no edge), and in the output; max_detour_count is the
 * greatest cnt[i] of step 2; device_ms is the time between the table's arrival on the device and the last kernel. */
typedef struct fsgpu_knn_optimize_stats {
    uint64_t rows, forward_edges, reverse_edges;
    uint64_t zero_in_degree_before, zero_in_degree_after;
    uint32_t max_detour_count, reserved;
    double device_ms;
} fsgpu_knn_optimize_stats;
fsgpu_status fsgpu_knn_graph_optimize(fsgpu_index *idx, const uint32_t *graph_rows, uint64_t graph_len, uint32_t graph_width,
                                      uint32_t out_degree, uint32_t *out_rows, fsgpu_knn_optimize_stats *stats);
/* SmoothConfig (smooth.rs:38-69): defaults alpha = 0.3, m = 10, mutual = 0; the reserved words must be 0. */
typedef struct fsgpu_smooth_config {
    float alpha;
    uint32_t m;
    uint32_t mutual;
    uint32_t reserved[5]; /* must be 0 */
} fsgpu_smooth_config;
fsgpu_status fsgpu_smooth_config_default(fsgpu_smooth_config *config);
/* neighbor_smooth / neighbor_smooth_ranked (smooth.rs:84-153, 176-276) in place, on the host.  graph_rows [graph_len, graph_width] is
 * a table of fsgpu_index_build_knn_graph (its out_rows).
 * DEVIATION, deliberate: the reference keys the pool and the graph by doc-id STRING; this function keys both by ROW (hits[i].index),
 * which is what the device builds and what a search returns.  Two rows with the same doc id are two nodes here.  A hit with
 * index >= graph_len — a WAL virtual row, or 0xffffffff — has no edges and is nobody's neighbour: WAL documents are isolated.
 *   identity (*out_applied = 0, nothing touched, nothing sorted): alpha non-finite or <= 0, m == 0, a NULL or empty graph, n == 0.
 *   pool: row -> score; a row that occurs twice counts with its LAST occurrence (the AHashMap insert).
 *   walk: for each hit the first min(m, graph_width) entries of its list, stopping at the first 0xffffffff; every walked entry
 *     counts as examined, in the pool or not; the in-pool neighbours' scores are summed into ONE f32 accumulator in list order;
 *     mean = sum / (float)count, or the hit's own score when no neighbour is in the pool;
 *     score' = (1.0f - alpha) * score + alpha * mean as two multiplies and an add, none of it fused.
 *   mutual != 0: a walked in-pool neighbour counts only if the hit's row occurs ANYWHERE in that neighbour's stored list — all
 *     graph_width columns, not the first m (the reference's reciprocity set is uncapped).
 *   resort != 0 sorts by VectorHit::cmp_rank, as fsgpu_apply_hubness_penalty does.  A NULL config means the defaults; non-zero
 *   reserved words are FSGPU_ERR_INVALID_CONFIG. */
fsgpu_status fsgpu_neighbor_smooth(fsgpu_scored_doc *hits, uint32_t n, const uint32_t *graph_rows, uint64_t graph_len,
                                   uint32_t graph_width, const fsgpu_smooth_config *config, int32_t resort, uint8_t *out_applied);

/* ---- graph ANN search over the k-NN table, with certified recall ---- */
/* The reference's `ann` feature: HnswIndex::knn_search_with_stats (crates/frankensearch-index/src/hnsw.rs:842-1330), which
 * TwoTierIndex::search_fast prefers when a sidecar exists, and the certificate that turns it on without a human sign-off
 * (recall_certificate.rs, HnswIndex::certify_ef_search, hnsw.rs:1354-1386).  The graph here is NOT an HNSW: it is the exact [N, m]
 * neighbour table of fsgpu_index_build_knn_graph, searched with a beam.  What is kept of the reference is the interface: k and ef per
 * call, the underfill fallback to the exact search (hnsw.rs:299-309, 1150-1190), the stats, the certificate.
 * THE ANSWER IS A PURE FUNCTION of (slab, live bitmap, table, query, parameters), returned bit for bit in any batch:
 *   scores  every score is the exact search's: dot_product_f16_bytes_f32 / dot_product_f32_bytes_f32 in the index's current hreduce
 *           order — the bits fsgpu_gather_dot returns for that row.
 *   order   the reference's total order (search.rs:91-126): score descending with NaN as -inf, row ascending.
 *   entry   the rows e_i = floor(i * N / n_entry), i < n_entry; the live ones are scored and become VISITED; the beam is the best ef
 *           of them, none expanded yet.
 *   step    take the first `expand` unexpanded beam entries in beam order (none: stop) and mark them expanded; walk each one's list
 *           in the table — the first `degree` columns, stopping at the first 0xffffffff; a walked row is ADMITTED if it lies inside
 *           the index, is live (the bitmap is read at search time: deletes made after the build are honoured) and is not visited;
 *           admitted rows become visited and are scored, a row reached twice in one step counts once; the beam becomes the best ef of
 *           (beam + admitted), entries keep their expanded flag.
 *   end     at most max_iters steps; the answer is the first min(k, |beam|) entries, rows and scores, and that count.  Entries of
 *           out_rows / out_scores past the count are unspecified.  Row ids are global (row_base is added, as in the table).
 * Visited is a set: nothing depends on insertion order, hash layout or which lane won a race.
 * FALLBACK (hnsw.rs:299-309): a query whose count is below min(k, live rows) is answered again by the handle's exact batched search
 * and flagged FSGPU_ANN_UNDERFILLED, or FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS when its count was 0.  Flag 0: the answer is the
 * approximate one.  AnnSearchStats::estimated_recall (0.9 + 0.1 log2(ef / k), which the reference itself calls ungrounded) is left
 * out: the certificate below replaces it.
 * LIMITS, checked before any launch (FSGPU_ERR_INVALID_CONFIG): 1 <= k <= ef <= 256; 1 <= expand <= 8; max_iters >= 1;
 * expand * degree <= 512 (the rows of one step); max_iters * expand * degree <= 4,096 (the visited set is an open-addressing table
 * of 8,192 rows in LDS, at most half full; entry rows do not occupy it: membership in the strided entry set is arithmetic);
 * n_entry <= 65,536 after clamping to N; dimension <= 16,384 (the query sits in LDS as f32).
 * HOW IT RUNS (ann_kernels.hip): one workgroup of 256 threads per query; a quad of lanes scores one row, 64 rows per pass; the beam
 * and the step's admitted keys are packed 64-bit keys in LDS, the step's keys are sorted with the block sort and merged into the
 * beam by rank; the expanded flags lie beside the keys.  Every table, list and row index is checked against N before it is used as
 * an address: the table is the caller's.  No inter-workgroup communication.  F16 and F32 slabs, every hreduce order, any dimension.
 * Out of scope: allow-bitmap filters, WAL entries and doc-id dedup (row-level, like fsgpu_search_topk), sharded handles. */
typedef struct fsgpu_ann fsgpu_ann;
typedef struct fsgpu_ann_config {
    uint32_t n_entry;   /* entry rows; clamped to record_count.  Default 1,024 */
    uint32_t degree;    /* columns of a list that are walked; 0 = the table's width.  Default 0 */
    uint32_t expand;    /* beam entries expanded per step, 1 .. 8.  Default 4 */
    uint32_t max_iters; /* steps at most, >= 1.  Default 64 */
    uint32_t reserved[4]; /* must be 0 */
} fsgpu_ann_config;
enum {
    FSGPU_ANN_APPROXIMATE = 0,
    FSGPU_ANN_UNDERFILLED = 1,                  /* AnnFallbackReason::Underfilled (hnsw.rs:304) */
    FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS = 2  /* AnnFallbackReason::EmptyDespiteIndexedPoints (hnsw.rs:308) */
};
/* AnnSearchStats (hnsw.rs:266-297) summed over one call.  For fsgpu_ann_certify_ef: summed over the launches of the sweep, with
 * ef_search the LARGEST ef that was launched. */
typedef struct fsgpu_ann_stats {
    uint64_t index_size;   /* record_count */
    uint32_t dimension;
    uint32_t ef_search;
    uint32_t k_requested;
    uint32_t launches;     /* launches of the ANN kernel */
    uint64_t queries;
    uint64_t approximate, underfilled, empty_despite_indexed_points; /* queries per flag value */
    uint64_t rows_scored;  /* entry rows and admitted rows */
    uint64_t steps;
    double device_ms;      /* the ANN kernel's launches, by device events (the fallback's exact search is not in it) */
} fsgpu_ann_stats;
fsgpu_status fsgpu_ann_config_default(fsgpu_ann_config *config);
/* HnswIndex::load over an index's table (hnsw.rs:700-840 is the sidecar loader): graph_rows [graph_len, graph_width] is the HOST
 * table fsgpu_index_build_knn_graph wrote (its out_rows, first_row 0), uploaded once to the index's device.  graph_len must equal
 * record_count and graph_width >= 1; a NULL config means the defaults.  The handle records fsgpu_index_generation: after a compaction
 * or a vacuum that moved rows every call on it is FSGPU_ERR_INVALID_CONFIG, as for an fsgpu_allow_bitmap.  The index must outlive the
 * handle. */
fsgpu_status fsgpu_ann_create(fsgpu_index *idx, const uint32_t *graph_rows, uint64_t graph_len, uint32_t graph_width,
                              const fsgpu_ann_config *config, fsgpu_ann **out);
void fsgpu_ann_destroy(fsgpu_ann *ann);
uint64_t fsgpu_ann_record_count(const fsgpu_ann *ann);
int32_t fsgpu_ann_device(const fsgpu_ann *ann);
/* HnswIndex::knn_search_with_stats (hnsw.rs:842-1330) for nq queries: queries [nq, query_len] f32, out_rows / out_scores [nq, k],
 * out_counts / out_flags [nq] (out_flags and stats may be NULL), HOST pointers; the call blocks.  query_len must equal the index's
 * dimension (FSGPU_ERR_DIMENSION_MISMATCH), as in fsgpu_search_topk_batched.  On any error nothing is written. */
fsgpu_status fsgpu_ann_search_batched(fsgpu_ann *ann, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t ef,
                                      uint32_t *out_rows, float *out_scores, uint32_t *out_counts, uint32_t *out_flags,
                                      fsgpu_ann_stats *stats);
/* The same with queries and outputs in the memory of the index's device (an encoder's output in, a reranker's input out); stats is
 * a host struct.  Same bits as the host form.  Blocks: the fallback decision is taken on the host. */
fsgpu_status fsgpu_ann_search_batched_device_queries(fsgpu_ann *ann, const float *queries_dev, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t ef, uint32_t *out_rows_dev, float *out_scores_dev,
                                                     uint32_t *out_counts_dev, uint32_t *out_flags_dev, fsgpu_ann_stats *stats);
/* A batch of one (hnsw.rs:842). */
fsgpu_status fsgpu_ann_search(fsgpu_ann *ann, const float *query, uint32_t query_len, uint32_t k, uint32_t ef, uint32_t *out_rows,
                              float *out_scores, uint32_t *out_count, uint32_t *out_flag, fsgpu_ann_stats *stats);
/* The stats of the last search or certify call on the handle. */
fsgpu_status fsgpu_ann_last_stats(const fsgpu_ann *ann, fsgpu_ann_stats *stats);

/* The recall certificates (recall_certificate.rs:50-230) restated in f64, on the host.  Non-finite entries are ignored.
 * conformal_recall_lower_bound (:50-73): the floor(alpha (n + 1))-th smallest recall (1-indexed) clamped to [0, 1]; 0 when that rank
 * is 0, the sample is empty or alpha is outside [0, 1). */
double fsgpu_conformal_recall_lower_bound(const double *recalls, uint64_t n, double alpha);
/* mean_recall_lower_bound (:88-102), Hoeffding: mean - sqrt(ln(1 / delta) / (2 n)) clamped to [0, 1]; the sum runs in array order. */
double fsgpu_mean_recall_lower_bound(const double *recalls, uint64_t n, double delta);
/* mean_recall_lower_bound_bernstein (:122-138), Maurer and Pontil: mean - sqrt(2 V ln(2 / delta) / n) - 7 ln(2 / delta) / (3 (n - 1))
 * with V the unbiased sample variance, clamped to [0, 1]; 0 for n < 2. */
double fsgpu_mean_recall_lower_bound_bernstein(const double *recalls, uint64_t n, double delta);
/* CertifiedEf (:143-152). */
typedef struct fsgpu_certified_ef {
    uint32_t ef_search;
    uint32_t meets_target;     /* certified_recall >= target */
    double certified_recall;
} fsgpu_certified_ef;
/* certified_min_ef (:165-191): calibration entry i is (efs[i], recalls[i][0 .. lens[i])).  In ascending ef (equal efs in the order
 * given) the first whose conformal bound meets the target; else the one with the highest bound (the first of equals), with
 * meets_target = 0.  n == 0 is FSGPU_ERR_INVALID_CONFIG (the reference's None). */
fsgpu_status fsgpu_certified_min_ef(const uint32_t *efs, const double *const *recalls, const uint64_t *lens, uint32_t n, double target,
                                    double alpha, fsgpu_certified_ef *out);
/* certified_min_ef_mean (:206-230): the same over the empirical-Bernstein bound of the mean. */
fsgpu_status fsgpu_certified_min_ef_mean(const uint32_t *efs, const double *const *recalls, const uint64_t *lens, uint32_t n,
                                         double target, double delta, fsgpu_certified_ef *out);
/* HnswIndex::certify_ef_search (hnsw.rs:1354-1386) through calibrate_certified_ef (recall_certificate.rs:259-292).  queries
 * [nq, dimension] are host values.  The exact top-k comes ONCE per query from the handle's exact batched search; the candidates are
 * de-duplicated and taken in ascending ef; a query's recall is recall_at_k_of over rows (hnsw.rs:3101-3112: the share of the exact
 * rows that the approximate answer holds, 1.0 when the exact answer is empty), and 0.0 when the query was flagged
 * (certified_ann_recall_sample, hnsw.rs:3114-3122).  The sweep stops at the first ef whose conformal bound meets the target: no ANN
 * launch happens at a larger ef.  sweep_out holds n_efs entries and receives one per ef measured (*n_swept); *chosen is the last of
 * them when it meets the target, else the entry with the highest bound.  Every candidate must satisfy k <= ef <= 256 and
 * n_efs >= 1, checked before any launch. */
fsgpu_status fsgpu_ann_certify_ef(fsgpu_ann *ann, const float *queries, uint32_t nq, const uint32_t *candidate_efs, uint32_t n_efs,
                                  uint32_t k, double target, double alpha, fsgpu_certified_ef *chosen, fsgpu_certified_ef *sweep_out,
                                  uint32_t *n_swept);

/* ---- IVF index: device k-means, probed-list search, certified nprobe ---- */
/* An inverted-file index over an index's rows (the reference pins a Lloyd k-means IVF in
 * crates/frankensearch-index/tests/ivf_recall_test.rs): the rows are partitioned by a coarse quantiser trained on the device and a
 * search scores only the lists nearest to the query.  THE INDEX AND EVERY ANSWER ARE PURE FUNCTIONS of their inputs, returned bit
 * for bit; only recall is statistical, and it is certified (fsgpu_ivf_certify_nprobe), never assumed.
 *   scope     F16 slabs whose dimension is a multiple of 8 and which the segmented gather scan covers; 1 <= nlist <= 65,536 and
 *             nlist <= the number of training rows; 0 <= iters <= 64; per call 1 <= k <= 256, 1 <= nprobe <= min(nlist, 256) and
 *             nprobe * k <= 16,384 (the per-query merge sorts a query's lists in LDS in one pass).  Everything else is
 *             FSGPU_ERR_INVALID_CONFIG (FSGPU_ERR_DIMENSION_MISMATCH for the query length), refused before any launch; nothing
 *             is written.  The handle records fsgpu_index_generation and the index's hreduce order at create and refuses every
 *             call once either has changed, as an fsgpu_allow_bitmap does.
 *   scores    row against centroid (training, assignment): the bits fsgpu_gather_dot(idx, centroid, [row]) returns —
 *             dot_product_f16_bytes_f32 in the index's hreduce order with the centroid as the f32 query.  Query against centroid
 *             (the coarse step): dot_product_f32_bytes_f32(centroid row, query) in the same order — what an F32 index over the
 *             [nlist, dim] centroid matrix answers.  Row against query: the exact search's bits.
 *   order     everywhere the reference's total order (search.rs:91-126): score descending with NaN as -inf, the lower id first —
 *             centroid ids and row ids alike.  A row whose every score is NaN goes to list 0.
 *   training  the training rows are the live rows among floor(i * N / n_train), i < n_train, ascending (n_train == 0 or >= N:
 *             every live row); T is their count.  Initial centroid c is init_centroids[c] (every value finite, else refused) or,
 *             with a NULL init_centroids, the f32 widening of training row number floor(c * T / nlist).  Then, iters times: every
 *             training row takes its best centroid; per list with members, taken in ascending row order, and per dimension d:
 *             s = the f64 sum of the widened values, SEQUENTIAL in that order; mean_d = s / count (f64); norm2 = the sequential
 *             f64 sum over ascending d of mean_d * mean_d (a multiply and an add); when norm2 is finite and > 0 the new value is
 *             (float)(mean_d / sqrt(norm2)), otherwise the centroid stays.  A list without members keeps its centroid
 *             (ivf_recall_test.rs:105-112).  Finally ALL live rows are assigned to the final centroids.
 *   index     list_offsets [nlist + 1] and list_rows: LOCAL row ids, ascending inside a list; dead rows are in no list.
 *   search    the nprobe best centroids; the candidates are the rows of their lists that are live NOW (deletes made after the
 *             build are honoured); the answer is the best min(k, |candidates|) by the exact score, row ids global (row_base
 *             added).  Lists are disjoint and keys unique: neither the order in which lists are scanned nor the batch position
 *             reaches the result, and nprobe == nlist is the exact search.  Entries past a count are unspecified.
 *   fallback  (hnsw.rs:299-309) a query whose count is below min(k, live rows) is answered again by the handle's exact batched
 *             search and flagged FSGPU_ANN_UNDERFILLED, or FSGPU_ANN_EMPTY_DESPITE_INDEXED_POINTS when its count was 0.
 * Out of scope: F32 slabs, allow-bitmap filters, WAL entries and doc-id dedup (row-level, like fsgpu_search_topk), sharded handles. */
typedef struct fsgpu_ivf fsgpu_ivf;
typedef struct fsgpu_ivf_config {
    uint32_t iters;       /* Lloyd iterations, 0 .. 64.  Default 8 */
    uint32_t reserved0;   /* must be 0 */
    uint64_t n_train;     /* strided training sample; 0 or >= record_count: every live row.  Default 0 */
    uint32_t reserved[4]; /* must be 0 */
} fsgpu_ivf_config;
typedef struct fsgpu_ivf_build_info {
    uint32_t iterations;
    uint32_t reserved0;
    uint64_t rows_trained;        /* T */
    uint64_t rows_changed_last;   /* training rows whose list in the last iteration differs from the one before (first: all) */
    uint64_t empty_lists, largest_list, smallest_list;   /* of the final lists */
    double assign_ms, update_ms, lists_ms;   /* device time per stage, summed over the iterations and the final assignment */
} fsgpu_ivf_build_info;
/* Summed over one call.  For fsgpu_ivf_certify_nprobe: summed over the searches of the sweep, with nprobe the LARGEST launched. */
typedef struct fsgpu_ivf_stats {
    uint64_t index_size;   /* record_count */
    uint32_t dimension;
    uint32_t nlist;
    uint32_t nprobe;
    uint32_t k_requested;
    uint32_t launches;     /* coarse searches and gather-scan launches */
    uint32_t reserved0;
    uint64_t queries;
    uint64_t approximate, underfilled, empty_despite_indexed_points; /* queries per flag value */
    uint64_t lists_probed; /* (query, list) pairs */
    uint64_t rows_scored;  /* the sum of the list lengths over all (query, list) pairs */
    double device_ms;      /* from the coarse search to the per-query merge, the host plan between them included */
} fsgpu_ivf_stats;
fsgpu_status fsgpu_ivf_config_default(fsgpu_ivf_config *config);
/* Trains the centroids and builds the lists on the index's device; blocks.  init_centroids: HOST [nlist, dimension] or NULL; a
 * NULL config means the defaults.  The index must outlive the handle. */
fsgpu_status fsgpu_ivf_create(fsgpu_index *idx, uint32_t nlist, const float *init_centroids, const fsgpu_ivf_config *config,
                              fsgpu_ivf **out);
void fsgpu_ivf_destroy(fsgpu_ivf *ivf);
uint64_t fsgpu_ivf_record_count(const fsgpu_ivf *ivf);
int32_t fsgpu_ivf_device(const fsgpu_ivf *ivf);
uint32_t fsgpu_ivf_nlist(const fsgpu_ivf *ivf);
/* out: HOST [nlist, dimension], the final centroids.  With iters = 0 and iters = 1 the two getters expose the assignment and the
 * update one launch at a time. */
fsgpu_status fsgpu_ivf_centroids(fsgpu_ivf *ivf, float *out);
/* out_offsets: HOST [nlist + 1]; out_rows: HOST [out_offsets[nlist]] (the live rows at create), either may be NULL. */
fsgpu_status fsgpu_ivf_lists(fsgpu_ivf *ivf, uint64_t *out_offsets, uint32_t *out_rows);
/* What the build did and what it cost. */
fsgpu_status fsgpu_ivf_build_stats(const fsgpu_ivf *ivf, fsgpu_ivf_build_info *stats);
/* The argument shapes of the fsgpu_ann_search* trio with nprobe for ef: HOST pointers / device pointers / a batch of one. */
fsgpu_status fsgpu_ivf_search_batched(fsgpu_ivf *ivf, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k, uint32_t nprobe,
                                      uint32_t *out_rows, float *out_scores, uint32_t *out_counts, uint32_t *out_flags,
                                      fsgpu_ivf_stats *stats);
fsgpu_status fsgpu_ivf_search_batched_device_queries(fsgpu_ivf *ivf, const float *queries_dev, uint32_t nq, uint32_t query_len,
                                                     uint32_t k, uint32_t nprobe, uint32_t *out_rows_dev, float *out_scores_dev,
                                                     uint32_t *out_counts_dev, uint32_t *out_flags_dev, fsgpu_ivf_stats *stats);
fsgpu_status fsgpu_ivf_search(fsgpu_ivf *ivf, const float *query, uint32_t query_len, uint32_t k, uint32_t nprobe, uint32_t *out_rows,
                              float *out_scores, uint32_t *out_count, uint32_t *out_flag, fsgpu_ivf_stats *stats);
/* The stats of the last search or certify call on the handle. */
fsgpu_status fsgpu_ivf_last_stats(const fsgpu_ivf *ivf, fsgpu_ivf_stats *stats);
/* fsgpu_ann_certify_ef with nprobe candidates: the exact top-k ONCE per query from the handle's exact batched search; the candidates
 * de-duplicated and taken in ascending order; recall_at_k_of over rows, 0.0 for a flagged query; the conformal bound after each;
 * no launch past the first nprobe that meets the target.  ef_search of fsgpu_certified_ef carries nprobe.  Every candidate must
 * satisfy the call's limits and n_probes >= 1, checked before any launch. */
fsgpu_status fsgpu_ivf_certify_nprobe(fsgpu_ivf *ivf, const float *queries, uint32_t nq, const uint32_t *candidate_nprobes,
                                      uint32_t n_probes, uint32_t k, double target, double alpha, fsgpu_certified_ef *chosen,
                                      fsgpu_certified_ef *sweep_out, uint32_t *n_swept);
/* The int8 list filter (opt-in, default off; off is the path and the stats described above).  On, every probed list is scored once
 * on the int8 matrix cores for all the queries that probe it, from a copy of the index's int8 filter rows laid out list by list; per
 * (query, list) slot only the rows that can still reach the slot's exact top k under the proven per-query bound delta of
 * fsgpu_index_int8_filter_bound are then scored exactly.  EVERY ANSWER IS BIT FOR BIT THE FILTER-OFF ANSWER, and every field of
 * fsgpu_ivf_stats but launches and device_ms is the filter-off value (rows_scored stays the sum of the list lengths).
 *   rule      slot (q, c), delta_q >= 0, L = the rows of list c live now, s_r = the int32 dot of q's codes with row r's.  |L| <= k:
 *             the candidates are L.  Otherwise t = the k-th largest s_r with multiplicity, m = ceil(2 delta_q), and the candidates
 *             are the rows of L with s_r >= t - m, ascending.  More than slot_cap (128) candidates: the slot overflows and is scored
 *             over its whole list.  A query with delta_q < 0 (non-finite, zero or overflowing; a slab the bound does not cover) is
 *             uncertified and takes the filter-off path inside the same call; so does a whole call with k > k_cap (64).
 *   handle    the cluster-ordered copy, the scale word, the statistics and the rotation it was built from are the handle's own: the
 *             index may rebuild or drop its filter copy afterwards.  fsgpu_ivf_certify_nprobe and the three searches honour the mode. */
#define FSGPU_IVF_LIST_FILTER_OFF  0
#define FSGPU_IVF_LIST_FILTER_INT8 1
/* INT8: builds the handle's cluster-ordered int8 copy on first use (blocks; builds the index's filter copy if need be).  An unknown
 * mode is FSGPU_ERR_INVALID_CONFIG: nothing is built, nothing changes. */
fsgpu_status fsgpu_ivf_set_list_filter(fsgpu_ivf *ivf, uint32_t mode);
uint32_t fsgpu_ivf_list_filter(const fsgpu_ivf *ivf);
/* Of the last search or certify call (summed over the sweep's searches); with the filter off everything per call is 0.  mode, rotated,
 * the caps, copy_bytes and build_ms are the handle's as it stands. */
typedef struct fsgpu_ivf_filter_stats {
    uint32_t mode;                /* FSGPU_IVF_LIST_FILTER_* */
    uint32_t rotated;             /* the handle's copy was made from a rotated filter copy */
    uint32_t slot_cap, k_cap;     /* 128, 64 */
    uint64_t scratch_cap;         /* int32 scores resident at once; a call above it runs in ranges */
    uint64_t copy_bytes;          /* of the ordered copy, padding included */
    double build_ms;              /* what building it cost on the device */
    uint64_t queries_filtered;    /* delta >= 0 */
    uint64_t queries_uncertified; /* delta < 0: the filter-off path inside the same call */
    uint64_t calls_above_k_cap;   /* 1: k > k_cap sent the whole call down the filter-off path */
    uint64_t slots_filtered;      /* slots the filter scored and selected from, the overflowed ones included */
    uint64_t slots_overflowed;    /* more than slot_cap candidates */
    uint64_t slots_above_scratch; /* slots of certified queries whose tile alone exceeds scratch_cap: scanned whole */
    uint64_t scratch_ranges;      /* score + selection launch pairs */
    uint64_t rows_filtered;       /* int8 dots: the sum of the list lengths, dead rows included, over slots_filtered */
    uint64_t rows_rescored;       /* exact dots made: candidates + the whole lists of every other slot (k > k_cap: rows_scored) */
    double filter_ms, select_ms, rescore_ms;   /* device time of the score launches, the selections, the exact scan and its merge */
    uint64_t rows_streamed;       /* rows of the ordered copy the score launches read: a list once per 16 member queries */
    uint64_t reserved[3];
} fsgpu_ivf_filter_stats;
fsgpu_status fsgpu_ivf_last_filter_stats(const fsgpu_ivf *ivf, fsgpu_ivf_filter_stats *out);

/* ---- MRL: truncated scan + full-dimension rescore ---- */
/* MrlSearchStats (crates/frankensearch-index/src/mrl.rs:122-139). */
typedef struct fsgpu_mrl_stats {
    uint32_t scan_dims, rescore_dims, candidates_rescored;
    uint64_t records_scanned;
    int32_t fell_back_to_full;
} fsgpu_mrl_stats;
/* VectorIndex::mrl_search_with_stats (mrl.rs:241-395) with MrlConfig{search_dims, rescore_dims, rescore_top_k}
 * (:55-115; 0 = full dimension / 3*k): phase 1 scores only the first search_dims dimensions of every live row (the
 * kernel reads that prefix of each row: N*search_dims*2 bytes instead of N*dim*2) and keeps the top rescore_top_k,
 * resident WAL entries join with their truncated f32 dot; phase 2 re-scores the candidates over rescore_dims and
 * returns the best k, best first (WAL hits at the virtual index record_count + i; no doc-id dedup, as the reference).
 * search_dims >= dimension falls back to the standard search; search_dims == 0 is FSGPU_ERR_INVALID_CONFIG.
 * out_rows / out_scores hold k entries; stats may be NULL. */
fsgpu_status fsgpu_search_mrl(fsgpu_index *idx, const float *query, uint32_t query_len, uint32_t k, uint32_t search_dims,
                              uint32_t rescore_dims, uint32_t rescore_top_k, uint32_t *out_rows, float *out_scores,
                              uint32_t *out_count, fsgpu_mrl_stats *stats);

/* fsgpu_search_mrl for nq queries at once (row-level results, no stats): the truncated scan of phase 1 runs on the matrix cores
 * for the whole batch (mfma_scan.hip / mfma_wide.hip over the strided prefix of every row: N*search_dims*2 bytes per 256-384
 * queries), phase 2 re-scores every query's rescore_top_k candidates in one launch.  Outputs as fsgpu_search_topk ([nq, k]
 * rows / scores, [nq] counts); hits equal fsgpu_search_mrl's for each query.  Resident WAL entries, rescore_top_k > 64,
 * k > 64 or unsupported search_dims (not 64 / 128 / 256) are answered query by query (*out_fallbacks, may be NULL). */
fsgpu_status fsgpu_search_mrl_batched(fsgpu_index *idx, const float *queries, uint32_t nq, uint32_t query_len, uint32_t k,
                                      uint32_t search_dims, uint32_t rescore_dims, uint32_t rescore_top_k, uint32_t *out_rows,
                                      float *out_scores, uint32_t *out_counts, uint32_t *out_fallbacks);

/* ---- dynamic batching of concurrent callers ---- */
/* The reference's seams are per-query calls made by many host threads at once (VectorIndex::search_top_k takes &self,
 * crates/frankensearch-index/src/search.rs:192; SyncEmbed::embed_sync, crates/frankensearch-core/src/traits.rs:401-582;
 * the MiniLM backends serialise callers on a mutex, crates/frankensearch-rerank/src/native_embedder.rs:40-50).  With
 * coalescing enabled, single-item calls that are in flight together (fsgpu_search_topk with nq = 1 and k <= 64 — filtered
 * callers share a batch when they pass the SAME allow bitmap, i.e. the same pointer; fsgpu_m2v_embed / fsgpu_bert_embed
 * with n = 1) are gathered into one batched launch: up to max_batch
 * items, waiting at most max_wait_us for the batch to fill.  Results are bit-identical to the unbatched calls.
 * max_batch = 0 turns it off (the default).  No threads are created: the first waiting caller runs the batch. */
fsgpu_status fsgpu_index_set_coalescing(fsgpu_index *idx, uint32_t max_batch, uint32_t max_wait_us);
fsgpu_status fsgpu_index_coalescing_stats(fsgpu_index *idx, uint64_t *batches, uint64_t *requests);
fsgpu_status fsgpu_m2v_set_coalescing(fsgpu_m2v *m, uint32_t max_batch, uint32_t max_wait_us);
fsgpu_status fsgpu_bert_set_coalescing(fsgpu_bert *m, uint32_t max_batch, uint32_t max_wait_us);

/* Environment switches (read once, at first use).
 * A default build reads eight:
 *   FSGPU_WIDE=0|2|3            batched main pass: 0 = queries in LDS (128 per pass), 2 / 3 = queries in registers (256 / 384 on f16 rows)
 *   FSGPU_WIDE_PRIO=off         the register-query kernels' split loop without its progress-ordered wave priority (same answers; for
 *                               timing the loop with and without it from one build)
 *   FSGPU_WIDE_SYNC=barrier     the register-query main pass on 128-row tiles with one block barrier per tile instead of its per-slot
 *                               counters (same answers; for timing the two forms from one build)
 *   FSGPU_WIDE_LAYOUT=sequential  the query groups of one register-query main-pass launch run one after the other on the whole grid
 *                               instead of side by side on a share of it each (same answers; for timing the two layouts from one build)
 *   FSGPU_FILTER=f16|i8         pin the candidate filter of the exact batched search (as fsgpu_index_set_batched_filter does per index)
 *   FSGPU_DEBUG_BATCHED         one line per batched search on stderr (fallback census)
 *   FSGPU_BERT_NO_GRAPH         the query-sized encoder calls launch eagerly instead of replaying a captured hipGraph
 *   FSGPU_DEBUG_GRAPH           say why a graph capture failed
 * Everything else is a tuning / A-B switch of the lab and exists only in builds with -DFSGPU_EXPERIMENTS
 * (FSGPU_BUILD_DEFS="-DFSGPU_EXPERIMENTS" python -m frankensearch_amd.build; scripts/exp_*, scripts/r03/): FSGPU_WIDE_OPT and
 * FSGPU_WIDE_DBG (options and timing skeletons of the wide main pass — skeleton answers are NOT valid), FSGPU_USE_160,
 * FSGPU_MFMA_SHAPE{,_I8}, FSGPU_RA, FSGPU_RB, FSGPU_ROUND, FSGPU_NO_SKIP_B, FSGPU_NO_REVERSE, FSGPU_I8F_GROWTH, FSGPU_WIDE_MAX,
 * FSGPU_SLOTS_B, FSGPU_SLOTS_MAIN, FSGPU_NO_WIDE_B, FSGPU_NO_ANCHOR, FSGPU_NO_BIG_POOL, FSGPU_NO_HEUR_B, FSGPU_HEUR_RANK,
 * FSGPU_RB_PCT, FSGPU_NO_GROUP_SAMPLE, FSGPU_WIDE_OPT, FSGPU_WIDE_DBG,
 * FSGPU_GRID_BLOCKS, FSGPU_I8_PER_CU, FSGPU_SELECT_SORT_ABOVE, FSGPU_BERT_GEMM_SHAPE, FSGPU_BERT_ATTN, FSGPU_BERT_NO_FUSED_LN,
 * FSGPU_BERT_NO_QUERY_PATH, FSGPU_BERT_GEMM_V1, FSGPU_BERT_SPLIT_FFN, FSGPU_BERT_SPLIT_AO, FSGPU_BERT_PACKED_MIN_TOKENS,
 * FSGPU_BERT_EMBED_V1. */

/* Bench fixtures, kernel timers and A/B switches (fsgpu_bench_fixture_device, fsgpu_index_set_profiling / _scan_time / _scan_stats /
 * _filter_stats, fsgpu_last_main_pass_kernel, fsgpu_index_set_variant) are not part of the drop-in surface: include/fsgpu_lab.h. */

#ifdef __cplusplus
}
#endif
#endif /* FSGPU_H */

"""ctypes binding of libfsgpu.so (the C ABI declared in include/fsgpu.h).

There is NO fallback: if the HIP library is missing this module raises at import of the symbol
table, and every compute entry point fails with FSGPU_ERR_NO_DEVICE when no GPU is visible.
"""
from __future__ import annotations

import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libfsgpu.so")

OK = 0
ERR_DIMENSION_MISMATCH = 1
ERR_INVALID_CONFIG = 2
ERR_INDEX_CORRUPTED = 3
ERR_INDEX_VERSION_MISMATCH = 4
ERR_IO = 5
ERR_DEVICE = 6
ERR_NO_DEVICE = 7
ERR_NULL_ARGUMENT = 8
ERR_EMBEDDING_FAILED = 9
ERR_MODEL_LOAD_FAILED = 10

ZERO_SIGNAL_NONE = 0
ZERO_SIGNAL_CALLER_REQUESTED_ZERO_K = 1
ZERO_SIGNAL_ZERO_NORM_QUERY = 2
ZERO_SIGNAL_FILTER_ELIMINATED_ALL = 3
ZERO_SIGNAL_NEWLY_CREATED_EMPTY = 4
ZERO_SIGNAL_ALL_TOMBSTONED = 5
ZERO_SIGNAL_WAL_ONLY_NO_LIVE_RECORDS = 6
ZERO_SIGNAL_NO_USABLE_VECTORS = 7

HREDUCE_SSE2 = 0
HREDUCE_AVX = 1
HREDUCE_SEQ = 2

_vp, _u32, _u64, _i32 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int32


class KnnOptimizeStats(C.Structure):   # fsgpu_knn_optimize_stats
    _fields_ = [("rows", C.c_uint64), ("forward_edges", C.c_uint64), ("reverse_edges", C.c_uint64), ("zero_in_degree_before", C.c_uint64),
                ("zero_in_degree_after", C.c_uint64), ("max_detour_count", C.c_uint32), ("reserved", C.c_uint32), ("device_ms", C.c_double)]


class KnnUpdateConfig(C.Structure):   # fsgpu_knn_update_config
    _fields_ = [("max_added_fraction", C.c_float), ("reserved", C.c_uint32 * 7)]


class KnnUpdateStats(C.Structure):   # fsgpu_knn_update_stats
    _fields_ = [("rows", C.c_uint64), ("dead", C.c_uint64), ("added", C.c_uint64), ("kept_clean", C.c_uint64), ("kept_dirty", C.c_uint64),
                ("searched_sources", C.c_uint64), ("join_pairs", C.c_uint64), ("join_entries", C.c_uint64), ("rebuilt", C.c_uint32),
                ("reserved", C.c_uint32), ("device_ms", C.c_double), ("join_ms", C.c_double)]


# name -> (restype, argtypes); must list every symbol include/fsgpu.h declares
SIGNATURES = {
    "fsgpu_version": (C.c_char_p, []),
    "fsgpu_device_count": (_i32, []),
    "fsgpu_last_error": (C.c_char_p, []),
    "fsgpu_last_main_pass_kernel": (C.c_char_p, []),
    "fsgpu_index_create": (_i32, [_i32, _u32, _u64, _vp, _vp, _u64, C.POINTER(_vp)]),
    "fsgpu_index_create_device": (_i32, [_i32, _u32, _u64, _vp, _vp, _u64, C.POINTER(_vp)]),
    "fsgpu_index_create_f32": (_i32, [_i32, _u32, _u64, _vp, _vp, _u64, C.POINTER(_vp)]),
    "fsgpu_index_create_f32_device": (_i32, [_i32, _u32, _u64, _vp, _vp, _u64, C.POINTER(_vp)]),
    "fsgpu_index_open_fsvi": (_i32, [C.c_char_p, _i32, C.POINTER(_vp)]),
    "fsgpu_index_destroy": (None, [_vp]),
    "fsgpu_index_record_count": (_u64, [_vp]),
    "fsgpu_index_dimension": (_u32, [_vp]),
    "fsgpu_index_set_hreduce": (_i32, [_vp, _i32]),
    "fsgpu_index_set_batched_filter": (_i32, [_vp, _i32]),
    "fsgpu_index_set_filter_rotation": (_i32, [_vp, _i32]),
    "fsgpu_index_filter_rotated": (_i32, [_vp]),
    "fsgpu_index_set_int8_latency": (_i32, [_vp, _i32]),
    "fsgpu_index_batched_filter_stats": (_i32, [_vp, _vp, _vp, _vp]),
    "fsgpu_index_int8_filter_bound": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_index_doc_id": (_i32, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "fsgpu_index_soft_delete": (_i32, [_vp, C.c_char_p, _u32, C.POINTER(_i32)]),
    "fsgpu_index_wal_append": (_i32, [_vp, C.c_char_p, _u32, _vp, _u32]),
    "fsgpu_index_wal_record_count": (_u64, [_vp]),
    "fsgpu_index_wal_append_batch": (_i32, [_vp, _u32, _vp, _vp, _vp, _u32]),
    "fsgpu_index_compact": (_i32, [_vp, C.c_char_p, _vp]),
    "fsgpu_index_vacuum": (_i32, [_vp, C.c_char_p, _vp]),
    "fsgpu_index_needs_compaction": (_i32, [_vp, _u64, C.c_double, C.POINTER(_i32)]),
    "fsgpu_index_needs_vacuum": (_i32, [_vp, C.POINTER(_i32)]),
    "fsgpu_index_tombstone_count": (_u64, [_vp]),
    "fsgpu_index_live_count": (_u64, [_vp]),
    "fsgpu_index_generation": (_u64, [_vp]),
    "fsgpu_index_compaction_gen": (_u32, [_vp]),
    "fsgpu_sharded_compact": (_i32, [_vp, C.c_char_p, _vp]),
    "fsgpu_sharded_vacuum": (_i32, [_vp, C.c_char_p, _vp]),
    "fsgpu_lab_index_set_compact_launch_rows": (_i32, [_vp, _u32]),
    "fsgpu_lab_index_set_compact_nt_stores": (_i32, [_vp, _i32]),
    "fsgpu_lab_index_last_rewrite": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(_u64)]),
    "fsgpu_lab_index_attach_synthetic_doc_ids": (_i32, [_vp]),
    "fsgpu_lab_hash_embed_stage_ms": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp]),
    "fsgpu_lab_device_copy_ms": (_i32, [_i32, _u64, _u32, C.POINTER(C.c_double)]),
    "fsgpu_index_set_live_bitmap": (_i32, [_vp, _vp]),
    "fsgpu_search_topk": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_search_topk_exact": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_allow_bitmap_create": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "fsgpu_allow_bitmap_destroy": (None, [_vp]),
    "fsgpu_allow_bitmap_allowed_rows": (_u64, [_vp]),
    "fsgpu_search_topk_filtered": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_search_topk_batched_filtered": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_multi_filtered": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_multi_filtered_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _u32, _vp, _vp, _vp, _vp, _vp,
                                                                        C.POINTER(_u32)]),
    "fsgpu_allow_bitmap_rows": (_i32, [_vp, _vp, _u64, C.POINTER(_u64)]),
    "fsgpu_index_multi_filter_stats": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_lab_multi_filter_plan": (_i32, [_u64, _vp, _u32, _vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_search_topk_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_packed_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_device_begin": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_i32)]),
    "fsgpu_search_topk_batched_device_end": (_i32, [_vp, _i32, C.POINTER(_u32)]),
    "fsgpu_search_topk_batched_device_end_late": (_i32, [_vp, _i32, C.POINTER(_u32), C.POINTER(_u32)]),
    "fsgpu_search_topk_packed_device": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "fsgpu_merge_topk_device": (_i32, [_i32, _vp, _u32, _u32, _u32, _u64, _u64, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_sharded_create": (_i32, [_vp, _u32, _u32, _u64, _vp, _vp, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_create_device": (_i32, [_vp, _u32, _u32, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_create_grouped": (_i32, [_vp, _u32, _u32, _u32, _u64, _vp, _vp, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_create_device_grouped": (_i32, [_vp, _u32, _u32, _u32, _vp, _vp, _vp, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_open_fsvi_grouped": (_i32, [C.c_char_p, _vp, _u32, _u32, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_query_groups": (_u32, [_vp]),
    "fsgpu_sharded_row_shards": (_u32, [_vp]),
    "fsgpu_sharded_set_int8_latency": (_i32, [_vp, _i32]),
    "fsgpu_sharded_search_parts": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_sharded_destroy": (None, [_vp]),
    "fsgpu_sharded_record_count": (_u64, [_vp]),
    "fsgpu_sharded_dimension": (_u32, [_vp]),
    "fsgpu_sharded_shard_count": (_u32, [_vp]),
    "fsgpu_sharded_exchange_mode": (_i32, [_vp]),
    "fsgpu_sharded_device": (_i32, [_vp, _u32]),
    "fsgpu_sharded_shard_range": (_i32, [_vp, _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_sharded_set_hreduce": (_i32, [_vp, _i32]),
    "fsgpu_sharded_search_topk": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp]),
    "fsgpu_sharded_search_topk_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_sharded_search": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_sharded_search_begin": (_i32, [_vp, _vp, C.POINTER(_u64)]),
    "fsgpu_sharded_search_end": (_i32, [_vp, _u64, _vp, _vp, _vp, _vp]),
    "fsgpu_sharded_quant_scale_max": (C.c_float, [_vp]),
    "fsgpu_sharded_set_coalescing": (_i32, [_vp, _u32, _u32]),
    "fsgpu_sharded_coalescing_stats": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_sharded_alignment_create": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "fsgpu_sharded_quality_scores_for_hits": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "fsgpu_sharded_open_fsvi": (_i32, [C.c_char_p, _vp, _u32, _i32, C.POINTER(_vp)]),
    "fsgpu_sharded_set_live_bitmap": (_i32, [_vp, _vp]),
    "fsgpu_sharded_soft_delete": (_i32, [_vp, C.c_char_p, _u32, C.POINTER(_i32)]),
    "fsgpu_sharded_wal_append": (_i32, [_vp, C.c_char_p, _u32, _vp, _u32]),
    "fsgpu_sharded_wal_record_count": (_u64, [_vp]),
    "fsgpu_sharded_doc_id": (_i32, [_vp, _u32, C.POINTER(_vp), C.POINTER(_u32)]),
    "fsgpu_sharded_search_hits": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_sharded_gather_dot": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "fsgpu_search_topk_classified": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32), C.POINTER(_i32)]),
    "fsgpu_search_topk_int8_two_pass": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_hits": (_i32, [_vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_hits_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_hits_batched_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_hits_two_pass_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_lab_index_wal_scores": (_i32, [_vp, _vp, _u32, _vp]),
    "fsgpu_gather_dot": (_i32, [_vp, _vp, _u32, _vp, _u32, _vp]),
    "fsgpu_lab_sort_keys_desc": (_i32, [_i32, _vp, _u64, _u64, _vp]),
    "fsgpu_bench_fixture_device": (_i32, [_i32, _u64, _u64, _u32, _u32, C.c_float, _u64, _i32, _vp, _vp]),
    "fsgpu_encode_f32_to_f16": (_i32, [_i32, _vp, _u64, _vp]),
    "fsgpu_widen_f16_to_f32": (_i32, [_i32, _vp, _u64, _vp]),
    "fsgpu_m2v_create": (_i32, [_i32, _vp, _u32, _u32, C.POINTER(_vp)]),
    "fsgpu_m2v_destroy": (None, [_vp]),
    "fsgpu_m2v_dimension": (_u32, [_vp]),
    "fsgpu_m2v_embed": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "fsgpu_bert_create": (_i32, [_i32, _vp, _vp, C.POINTER(_vp)]),
    "fsgpu_bert_create_safetensors": (_i32, [_i32, _vp, _u64, C.c_float, C.POINTER(_vp)]),
    "fsgpu_bert_create_ex": (_i32, [_i32, _vp, _vp, _vp, C.POINTER(_vp)]),
    "fsgpu_bert_create_safetensors_ex": (_i32, [_i32, _vp, _u64, C.c_float, _vp, C.POINTER(_vp)]),
    "fsgpu_bert_linear_format": (_u32, [_vp]),
    "fsgpu_lab_linear_int8_dynamic": (_i32, [_i32, _vp, _vp, _vp, _u32, _u32, _u32, _vp]),
    "fsgpu_lab_bert_stage": (_i32, [_i32, _vp]),   # (fsgpu_lab_bert_stage_args: BertStageArgs below)
    "fsgpu_lab_bert_int8_stage": (_i32, [_i32, _vp]),   # (fsgpu_lab_bert_int8_stage_args: BertInt8StageArgs below)
    "fsgpu_lab_bert_short_stage": (_i32, [_i32, _vp]),   # (fsgpu_lab_bert_short_args: BertShortArgs below)
    "fsgpu_lab_scan_stage": (_i32, [_i32, _vp]),   # (fsgpu_lab_scan_stage_args: ScanStageArgs below)
    "fsgpu_lab_scan_stage_check": (_i32, [_vp]),
    "fsgpu_lab_scan_planner_shape": (_i32, [_i32, _i32]),
    "fsgpu_lab_select": (_i32, [_i32, _vp]),   # (fsgpu_lab_select_args: SelectLabArgs below)
    "fsgpu_lab_select_check": (_i32, [_vp]),
    "fsgpu_lab_lone_stage": (_i32, [_i32, _vp]),   # (fsgpu_lab_lone_stage_args: LoneStageArgs below)
    "fsgpu_lab_lone_stage_check": (_i32, [_vp]),
    "fsgpu_bert_destroy": (None, [_vp]),
    "fsgpu_bert_embed_device": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "fsgpu_m2v_embed_device": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "fsgpu_search_topk_batched_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_int8_two_pass_batched_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_device_malloc": (_i32, [_i32, _u64, C.POINTER(_vp)]),
    "fsgpu_device_free": (_i32, [_i32, _vp]),
    "fsgpu_bert_device": (_i32, [_vp]),
    "fsgpu_m2v_device": (_i32, [_vp]),
    "fsgpu_index_device": (_i32, [_vp]),
    "fsgpu_bert_dimension": (_u32, [_vp]),
    "fsgpu_bert_embed": (_i32, [_vp, _vp, _vp, _u32, _vp]),
    "fsgpu_reranker_create": (_i32, [_i32, _vp, _vp, C.POINTER(_vp)]),
    "fsgpu_reranker_create_safetensors": (_i32, [_i32, _vp, _u64, C.c_float, C.POINTER(_vp)]),
    "fsgpu_reranker_destroy": (None, [_vp]),
    "fsgpu_reranker_device": (_i32, [_vp]),
    "fsgpu_reranker_max_length": (_u32, [_vp]),
    "fsgpu_reranker_score": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp]),
    "fsgpu_index_builder_create": (_i32, [_i32, _u32, C.c_char_p, C.c_char_p, _vp, C.POINTER(_vp)]),   # (options: index_builder._Options)
    "fsgpu_index_builder_destroy": (None, [_vp]),
    "fsgpu_index_builder_record_count": (_u64, [_vp]),
    "fsgpu_index_builder_add": (_i32, [_vp, _u64, _vp, _vp, _vp, _u32, C.POINTER(_u64)]),
    "fsgpu_index_builder_add_device": (_i32, [_vp, _u64, _vp, _vp, _vp, _u32, _vp, C.POINTER(_u64)]),
    "fsgpu_index_builder_add_bert": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u64)]),
    "fsgpu_index_builder_add_m2v": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u64)]),
    "fsgpu_index_builder_add_hash": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u64)]),
    "fsgpu_hash_create": (_i32, [_i32, _u32, _i32, _u64, _vp, C.POINTER(_vp)]),
    "fsgpu_hash_destroy": (None, [_vp]),
    "fsgpu_hash_dimension": (_u32, [_vp]),
    "fsgpu_hash_device": (_i32, [_vp]),
    "fsgpu_hash_embed": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_hash_embed_device": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_lab_wordpiece_encode_stage_ms": (_i32, [_vp, _vp, _vp, _u32, _i32, _u32, _vp, _u64, _vp, _vp]),
    "fsgpu_wordpiece_create": (_i32, [_i32, _vp, C.POINTER(_vp)]),
    "fsgpu_wordpiece_destroy": (None, [_vp]),
    "fsgpu_wordpiece_device": (_i32, [_vp]),
    "fsgpu_wordpiece_vocab_size": (_u32, [_vp]),
    "fsgpu_wordpiece_encode": (_i32, [_vp, _vp, _vp, _u32, _i32, _u32, _vp, _u64, _vp, _vp, C.POINTER(_u64), C.POINTER(_u32)]),
    "fsgpu_wordpiece_encode_device": (_i32, [_vp, _vp, _vp, _u32, _i32, _u32, _vp, _u64, _vp, _vp, C.POINTER(_u64), C.POINTER(_u32)]),
    "fsgpu_wordpiece_encode_pairs": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, C.POINTER(_u64),
                                            C.POINTER(_u32)]),
    "fsgpu_wordpiece_encode_pairs_device": (_i32, [_vp, _vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _u64, _vp, _vp, C.POINTER(_u64),
                                                   C.POINTER(_u32)]),
    "fsgpu_bert_embed_texts": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(_u32)]),
    "fsgpu_bert_embed_texts_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, C.POINTER(_u32)]),
    "fsgpu_reranker_score_texts": (_i32, [_vp, _vp, _vp, _u32, _vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_m2v_embed_texts": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, C.POINTER(_u32)]),
    "fsgpu_m2v_embed_texts_device": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, C.POINTER(_u32)]),
    "fsgpu_index_builder_finish": (_i32, [_vp, C.c_char_p, C.POINTER(_vp), _vp]),   # (stats: index_builder._Stats)
    "fsgpu_rerank_apply": (_i32, [_vp, _u32, _vp, _vp, _u32, _u32, _u32, _i32, C.c_float, _vp]),
    "fsgpu_mmr_config_default": (_i32, [_vp]),
    "fsgpu_mmr_rerank": (_i32, [_vp, _vp, _vp, _u32, _u32, C.c_double, _u32, _vp, C.POINTER(_u32), _vp]),
    "fsgpu_index_vector_at_f32": (_i32, [_vp, _u32, _vp]),
    "fsgpu_index_mmr_rerank": (_i32, [_vp, _vp, _vp, _u32, _u32, _vp, _vp, C.POINTER(_u32), _vp]),
    "fsgpu_index_mmr_rerank_batched": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp]),
    "fsgpu_index_mmr_rerank_docs": (_i32, [_vp, _vp, _u32, _vp, _vp, C.POINTER(C.c_uint8)]),
    "fsgpu_two_tier_mmr_rerank": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _vp, C.POINTER(C.c_uint8)]),
    "fsgpu_hubness_config_default": (_i32, [_vp]),
    "fsgpu_query_hubness": (_i32, [_vp, _vp, _u64, _vp, _vp, _u32, _u32, _i32, _vp]),
    "fsgpu_apply_hubness_penalty": (_i32, [_vp, _u32, _vp, _u64, _vp, _i32, C.POINTER(C.c_uint8)]),
    "fsgpu_index_compute_query_hubness": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "fsgpu_sharded_compute_query_hubness": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp]),
    "fsgpu_lab_index_query_hubness_topk": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp]),
    "fsgpu_index_build_knn_graph": (_i32, [_vp, _u64, _u64, _u32, _vp, _vp]),
    "fsgpu_sharded_build_knn_graph": (_i32, [_vp, _u64, _u64, _u32, _vp, _vp]),
    "fsgpu_lab_index_knn_build_stats": (_i32, [_vp, _vp]),
    "fsgpu_knn_graph_optimize": (_i32, [_vp, _vp, _u64, _u32, _u32, _vp, _vp]),
    "fsgpu_lab_knn_update_join": (_i32, [_i32, _vp, _u32, _u32, _u32, _i32, _u32, _vp, _vp, _vp, _vp, _u32]),
    "fsgpu_knn_update_config_default": (_i32, [_vp]),
    "fsgpu_index_update_knn_graph": (_i32, [_vp, _u32, _vp, _vp, _u64, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_index_rewrite_sources": (_i32, [_vp, _vp, C.POINTER(_u64), C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_ann_config_default": (_i32, [_vp]),
    "fsgpu_ann_create": (_i32, [_vp, _vp, _u64, _u32, _vp, C.POINTER(_vp)]),
    "fsgpu_ann_destroy": (None, [_vp]),
    "fsgpu_ann_record_count": (_u64, [_vp]),
    "fsgpu_ann_device": (_i32, [_vp]),
    "fsgpu_ann_search_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ann_search_batched_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ann_search": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ann_last_stats": (_i32, [_vp, _vp]),
    "fsgpu_ann_certify_ef": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, C.c_double, C.c_double, _vp, _vp, _vp]),
    "fsgpu_ivf_config_default": (_i32, [_vp]),
    "fsgpu_ivf_create": (_i32, [_vp, _u32, _vp, _vp, C.POINTER(_vp)]),
    "fsgpu_ivf_destroy": (None, [_vp]),
    "fsgpu_ivf_record_count": (_u64, [_vp]),
    "fsgpu_ivf_device": (_i32, [_vp]),
    "fsgpu_ivf_nlist": (_u32, [_vp]),
    "fsgpu_ivf_centroids": (_i32, [_vp, _vp]),
    "fsgpu_ivf_lists": (_i32, [_vp, _vp, _vp]),
    "fsgpu_ivf_build_stats": (_i32, [_vp, _vp]),
    "fsgpu_ivf_search_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ivf_search_batched_device_queries": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ivf_search": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp, _vp]),
    "fsgpu_ivf_last_stats": (_i32, [_vp, _vp]),
    "fsgpu_ivf_certify_nprobe": (_i32, [_vp, _vp, _u32, _vp, _u32, _u32, C.c_double, C.c_double, _vp, _vp, _vp]),
    "fsgpu_ivf_set_list_filter": (_i32, [_vp, _u32]),
    "fsgpu_ivf_list_filter": (_u32, [_vp]),
    "fsgpu_ivf_last_filter_stats": (_i32, [_vp, _vp]),
    "fsgpu_lab_ivf_filter_stage": (_i32, [_vp, _vp]),
    "fsgpu_lab_ivf_filter_set_scratch": (_i32, [_vp, _u64]),
    "fsgpu_lab_ivf_filter_score_plan": (_i32, [_u32, _vp, _vp, _u64, _u32, _vp, _vp, _u32, _vp, _vp, _vp]),
    "fsgpu_lab_ivf_filter_scan_plan": (_i32, [_u32, _vp, _vp, _vp, _vp, _u32, _u32, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_conformal_recall_lower_bound": (C.c_double, [_vp, _u64, C.c_double]),
    "fsgpu_mean_recall_lower_bound": (C.c_double, [_vp, _u64, C.c_double]),
    "fsgpu_mean_recall_lower_bound_bernstein": (C.c_double, [_vp, _u64, C.c_double]),
    "fsgpu_certified_min_ef": (_i32, [_vp, _vp, _vp, _u32, C.c_double, C.c_double, _vp]),
    "fsgpu_certified_min_ef_mean": (_i32, [_vp, _vp, _vp, _u32, C.c_double, C.c_double, _vp]),
    "fsgpu_smooth_config_default": (_i32, [_vp]),
    "fsgpu_neighbor_smooth": (_i32, [_vp, _u32, _vp, _u64, _u32, _vp, _i32, C.POINTER(C.c_uint8)]),
    "fsgpu_rrf_fuse": (_i32, [_vp, _u32, _vp, _u32, C.c_double, C.c_double, C.c_double, _i32, _u32, _u32, _vp,
                              C.POINTER(_u32)]),
    "fsgpu_blend_two_tier": (_i32, [_vp, _u32, _vp, _u32, C.c_float, _vp, C.POINTER(_u32)]),
    "fsgpu_blend_two_tier_aligned": (_i32, [_vp, _u32, _vp, _vp, C.c_float, _vp, C.POINTER(_u32)]),
    "fsgpu_alignment_create": (_i32, [_vp, _vp, C.POINTER(_vp)]),
    "fsgpu_alignment_destroy": (None, [_vp]),
    "fsgpu_alignment_kind": (_i32, [_vp]),
    "fsgpu_alignment_quality_row": (C.c_int64, [_vp, _u64]),
    "fsgpu_alignment_unmatched_quality_docs": (_u64, [_vp]),
    "fsgpu_quality_scores_for_hits": (_i32, [_vp, _vp, _vp, _vp, _u32, _vp, _u32, _vp, _vp]),
    "fsgpu_quality_scores_for_hits_batched": (_i32, [_vp, _vp, _vp, _vp, _u32, _u32, _vp, _vp, _vp, _vp]),
    "fsgpu_index_set_after_enqueue_hook": (_i32, [_vp, _vp, _vp]),
    "fsgpu_index_set_profiling": (_i32, [_vp, _i32]),
    "fsgpu_index_scan_time": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(_u64), _i32]),
    "fsgpu_search_topk_int8_two_pass_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_4bit_two_pass_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_topk_4bit_two_pass": (_i32, [_vp, _vp, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_fsvi_write": (_i32, [C.c_char_p, C.c_char_p, C.c_char_p, _u32, _u64, _vp, _vp, _vp, C.c_uint8, _i32]),
    "fsgpu_fsvi_write_quant": (_i32, [C.c_char_p, C.c_char_p, C.c_char_p, _u32, _u64, _vp, _vp, _vp, C.c_uint8, _i32,
                               C.c_uint8]),
    "fsgpu_search_mrl_batched": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _u32, _vp, _vp, _vp, C.POINTER(_u32)]),
    "fsgpu_search_mrl": (_i32, [_vp, _vp, _u32, _u32, _u32, _u32, _u32, _vp, _vp, C.POINTER(_u32), _vp]),
    "fsgpu_index_set_coalescing": (_i32, [_vp, _u32, _u32]),
    "fsgpu_index_coalescing_stats": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_m2v_set_coalescing": (_i32, [_vp, _u32, _u32]),
    "fsgpu_bert_set_coalescing": (_i32, [_vp, _u32, _u32]),
    "fsgpu_index_scan_stats": (_i32, [_vp, C.POINTER(C.c_double), C.POINTER(_u64), C.POINTER(_u64), _i32]),
    "fsgpu_index_allow_bitmap_for_hashes": (_i32, [_vp, C.POINTER(_u64), _u32, C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_index_filter_stats": (_i32, [_vp, C.POINTER(_u64), C.POINTER(_u64)]),
    "fsgpu_index_set_variant": (_i32, [_vp, _i32]),
}



class BertStageArgs(C.Structure):
    """fsgpu_lab_bert_stage_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("stage", "form", "epilogue", "m", "n", "k", "hidden", "inter", "n_docs", "vocab", "max_pos")] + [
        ("eps", C.c_float), ("scale", C.c_float), ("offsets", _vp), ("ids", _vp), ("positions", _vp), ("types", _vp),
        ("in_", _vp * 12), ("out0", _vp), ("out1", _vp)]


class BertInt8StageArgs(C.Structure):
    """fsgpu_lab_bert_int8_stage_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("stage", "form", "epilogue", "m", "n", "k", "hidden", "vocab", "max_pos")] + [
        ("eps", C.c_float), ("ids", _vp), ("positions", _vp), ("codes", _vp), ("in_", _vp * 5), ("out_f32", _vp), ("out_codes", _vp),
        ("out_scales", _vp)]


class BertShortArgs(C.Structure):
    """fsgpu_lab_bert_short_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("stage", "form", "m", "n_docs", "hidden", "inter", "heads", "layers", "vocab", "max_pos")] + [
        ("eps", C.c_float), ("scale", C.c_float), ("offsets", _vp), ("ids", _vp), ("positions", _vp),
        ("in_", _vp * 8), ("layer_in", _vp), ("out0", _vp), ("out1", _vp)]


class ScanStageArgs(C.Structure):
    """fsgpu_lab_scan_stage_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("kernel", "variant", "stage", "elem_bytes", "dim", "nrows", "row_stride", "row_base",
                                          "grid", "groups", "side_by_side", "reverse", "group_stride", "group_count", "slots", "spill_cap",
                                          "nq_pad", "want_counts", "nq", "max_norm_bits", "bits", "reserved")] + [
        (name, _vp) for name in ("slab", "live", "allow", "queries", "tau", "queries_f32", "cand", "cand_count", "spill", "spill_count",
                                 "overflow", "dense", "prepared", "delta")]


class SelectLabArgs(C.Structure):
    """fsgpu_lab_select_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("kernel", "nq", "valid_queries", "k")] + [("q_stride", _u64), ("shard_pitch", _u64)] + [
        (name, _u32) for name in ("l_stride", "nlists", "list_len", "extra_len", "spill_cap", "reset_spill", "take_topk", "heur_rank", "big_pool",
                                  "dim", "nrows", "row_base", "row_stride", "query_stride")] + [("hreduce", _i32)] + [
        (name, _u32) for name in ("k_out", "out_stride", "cand_out_stride", "slab_f32", "nentries", "rank_only", "nshards", "cc")] + [
        (name, _vp) for name in ("lists", "list_counts", "extra", "spill", "exact_lists", "delta", "anchor_unit", "tau_floor_in", "slab", "live",
                                 "allow", "queries", "spill_count", "pool_flag", "tau_out", "tau_floor_out", "pool_out", "cand_counts",
                                 "overflow", "out_rows", "out_scores", "out_packed", "out_counts", "cand_approx_out", "cand_exact_out")]


class LoneStageArgs(C.Structure):
    """fsgpu_lab_lone_stage_args of include/fsgpu_lab.h."""
    _fields_ = [(name, _u32) for name in ("kind", "nq", "tier", "dim", "nrows", "row_stride", "row_base", "k", "grid", "force_runtime_dim",
                                          "plain_loads")] + [("hreduce", _i32)] + [
        (name, _u32) for name in ("bitmap_words", "nlists", "list_len", "l_stride", "out_stride", "lists_sorted")] + [("q_stride", _u64)] + [
        (name, _vp) for name in ("slab", "live", "allow", "queries", "partial", "lists", "out_rows", "out_scores", "out_packed", "out_counts")]


_lib = None


def _share_torch_hip_runtime() -> None:
    """PyTorch-ROCm wheels bundle their own copies of the ROCm runtime libraries (libamdhip64, librccl, hsa-runtime, ...) under
    the SONAMEs libfsgpu.so also resolves.  Whichever copy of a library is loaded first serves the whole process: with the system
    HIP runtime first, a later `import torch` finds no GPU; with only SOME of the system copies first (libfsgpu loaded, then torch
    loading the rest of its own set) the process has been seen to abort in the libraries' exit handlers ("double free or
    corruption" after `pytest tests/test_gpu_sharded.py` alone, round 5 — the whole suite, where an earlier test file imports
    torch first, was fine).  When torch is installed, import it BEFORE libfsgpu.so is loaded, so that the order of imports in the
    caller does not matter (bench.py / sharded.py hand torch device pointers to this library anyway).  Loading RCCL alone ahead of
    time is not an option: without a GPU its own exit handlers abort."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    try:
        import torch  # noqa: F401
        return
    except Exception:   # a broken torch install: fall back to its HIP runtime alone
        pass
    cand = os.path.join(os.path.dirname(spec.origin), "lib", "libamdhip64.so")
    if os.path.exists(cand):
        try:
            C.CDLL(cand, mode=C.RTLD_GLOBAL)
        except OSError:
            pass  # fall back to the loader's own resolution


def lib() -> C.CDLL:
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                f"{LIB_PATH} is missing: build it with `python -m frankensearch_amd.build` "
                "(the HIP library is the product; there is no CPU fallback)")
        _share_torch_hip_runtime()
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the ABI and the header drift apart
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def last_error() -> str:
    return (lib().fsgpu_last_error() or b"").decode("utf-8", "replace")

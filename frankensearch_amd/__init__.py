"""frankensearch_amd — MI355X (gfx950) semantic tier for frankensearch.

The product is the HIP library `libfsgpu.so` (C ABI in include/fsgpu.h); this package is the thin
host-side mirror of the reference's VectorIndex / embedder interfaces used by tests and bench.py.
"""
from . import _lib
from .embed import HashEmbedder, Model2VecEmbedder, NativeEmbedder, WordPieceTokenizer, bert_codepoint_table, python_alnum_bitmap
from .errors import (DeviceError, DimensionMismatch, IndexCorrupted, IndexVersionMismatch, InvalidConfig, IoError,
                     ModelLoadFailed, NoDevice, SearchError)
from .index import (ClassifiedHits, CompactionStats, VacuumStats, NativeShardedIndex, VectorHit, VectorIndex, encode_f32_to_f16, pack_bitmap, widen_f16_to_f32,
                    write_fsvi)
from .index_builder import IndexBuilder, IndexBuildStats
from .two_tier import TwoTierIndexBuilder
from .hubness import HubnessConfig, apply_hubness_penalty, compute_query_hubness
from .smooth import SmoothConfig, neighbor_smooth, neighbor_smooth_ranked
from .mmr import MmrConfig, mmr_rerank, mmr_step
from .ann import (AnnConfig, AnnIndex, AnnStats, CertifiedEf, certified_min_ef, certified_min_ef_mean, conformal_recall_lower_bound,
                  mean_recall_lower_bound, mean_recall_lower_bound_bernstein)
from .ivf import IvfBuildStats, IvfConfig, IvfFilterStats, IvfIndex, IvfStats
from .rerank import PURE_REORDER, RRF_COMBINE, NativeReranker, RerankCandidate, RerankScore, rerank_step

__all__ = ["write_fsvi", "IndexBuilder", "IndexBuildStats", "TwoTierIndexBuilder", "VectorIndex", "NativeShardedIndex", "VectorHit", "ClassifiedHits", "CompactionStats", "VacuumStats", "Model2VecEmbedder", "NativeEmbedder", "HashEmbedder", "python_alnum_bitmap", "WordPieceTokenizer", "bert_codepoint_table", "NativeReranker",
           "RerankCandidate", "RerankScore", "rerank_step", "MmrConfig", "mmr_rerank", "mmr_step", "AnnConfig", "AnnIndex", "AnnStats", "IvfConfig", "IvfIndex", "IvfStats", "IvfBuildStats", "IvfFilterStats", "CertifiedEf", "certified_min_ef", "certified_min_ef_mean",
           "conformal_recall_lower_bound", "mean_recall_lower_bound", "mean_recall_lower_bound_bernstein", "HubnessConfig", "compute_query_hubness", "apply_hubness_penalty", "SmoothConfig", "neighbor_smooth", "neighbor_smooth_ranked", "PURE_REORDER", "RRF_COMBINE", "SearchError", "DimensionMismatch",
           "InvalidConfig", "IndexCorrupted", "IndexVersionMismatch", "IoError", "DeviceError", "NoDevice", "ModelLoadFailed",
           "encode_f32_to_f16", "widen_f16_to_f32", "pack_bitmap", "_lib"]

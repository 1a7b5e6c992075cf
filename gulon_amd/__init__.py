"""gulon_amd: MI355X-native ANN index build + query path behind Gulon's
Index / ProductQuantizer / KMeans API (host mirror over libgulon_hip.so)."""
from . import native
from .coder import Coder, width_for_clusters
from .index import DevicePQIndex, Index, PQIndex, PQIndexView, Result, SortedIndex, exact_nearest_neighbours, prepare_query, tune_live
from .grouped import GroupedIndex, GroupedVectors, LimitGroups, LimitVectors, group
from .kmeans import KMeans
from .kmeans import Config as KMeansConfig
from .matrix import DeviceMatrix, Matrix
from .product_quantizer import EncodedMatrix, ProductQuantizer, Quantizer
from .product_quantizer import Config as ProductQuantizerConfig
from .vectors import Vectors, subvector_bounds, subvectors
from .word_vectors import (DeviceWordVectors, GroupedWordVectors, KeyedIndex, KeyIndexGrouped, KeyIndexSorted,
                           WordVectors, read_word2vec, read_word2vec_device)
from .build import build_index
from .word_index import WordIndex, WordResult
from .refine import RefinedIndex, refine_topk
from .exact import ExactIndex, ExactWordIndex
from .fine import FineRefinedIndex, build_fine_index, refine_codes_topk, row_residuals
from .inspect import IndexReport, reference_quality
from .update import UpdatePlan, plan_update
from .expressions import (COSMUL_EPS, Expression, Term, compose_reference, cosmul_reference, parse_expression,
                          partition_by_operands)
from .rotation import RotatedWordIndex, Rotation, rotate_reference, train_rotation
from .analogies import AnalogyReport, evaluate_analogies, read_questions
from .similarity import (SimilarityReport, evaluate_pairs, pair_distance_reference, rank_sums, rank_sums_reference,
                         read_pairs, spearman)
from .csls import (DeviceOffsets, TranslationReport, csls_offsets, evaluate_dictionary, mean_similarity,
                   mean_similarity_reference, offset_query_reference, read_dictionary, translate_words,
                   translation_scores)
from .ranks import RankReport, evaluate_dictionary_ranks, rank_query_reference
from .alignment import (induce_matches, mutual_rows, mutual_rows_reference, pair_moment, pair_moment_reference,
                        seed_alignment, train_alignment)
from .csls import isf_offsets
from .softmax import isf_offsets_from, isf_probabilities, logsumexp_reference

__all__ = ["native", "GroupedIndex", "GroupedVectors", "LimitGroups", "LimitVectors", "group", "Coder", "width_for_clusters", "Index", "PQIndex", "PQIndexView", "DevicePQIndex", "Result", "SortedIndex",
           "exact_nearest_neighbours", "prepare_query", "tune_live", "KMeans", "KMeansConfig", "DeviceMatrix", "Matrix",
           "EncodedMatrix", "ProductQuantizer", "Quantizer", "ProductQuantizerConfig", "Vectors",
           "subvector_bounds", "subvectors", "GroupedWordVectors", "KeyedIndex", "KeyIndexGrouped", "KeyIndexSorted",
           "WordVectors", "read_word2vec", "WordIndex", "WordResult", "DeviceWordVectors", "read_word2vec_device",
           "build_index", "RefinedIndex", "refine_topk", "Expression", "Term", "compose_reference", "parse_expression",
           "partition_by_operands", "IndexReport", "reference_quality", "UpdatePlan", "plan_update", "FineRefinedIndex", "build_fine_index",
           "refine_codes_topk", "row_residuals", "Rotation", "RotatedWordIndex", "train_rotation", "rotate_reference",
           "ExactIndex", "ExactWordIndex", "AnalogyReport", "evaluate_analogies", "read_questions",
           "COSMUL_EPS", "cosmul_reference", "SimilarityReport", "evaluate_pairs", "read_pairs",
           "pair_distance_reference", "rank_sums", "rank_sums_reference", "spearman", "DeviceOffsets",
           "TranslationReport", "csls_offsets", "evaluate_dictionary", "mean_similarity", "mean_similarity_reference",
           "offset_query_reference", "read_dictionary", "translate_words", "translation_scores",
           "induce_matches", "mutual_rows", "mutual_rows_reference", "pair_moment", "pair_moment_reference",
           "seed_alignment", "train_alignment", "RankReport", "evaluate_dictionary_ranks", "rank_query_reference",
           "isf_offsets", "isf_offsets_from", "isf_probabilities", "logsumexp_reference"]

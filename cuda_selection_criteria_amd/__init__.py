"""MI355X-native all-pairs SuperMinHash/HLL sketch selection (drop-in for the hot path of
sanhue903/CUDA_Selection_Criteria: `selection` / `time_smh_cuda`).

Python here is plumbing only (device memory via torch, torch.distributed for the multi-GPU gather,
ctypes bindings); the product is csrc/ (HIP kernels + C ABI in include/selection_hip.h, C++ host code).
"""
from ._lib import (ALGO_AUTO, ALGO_HASHJOIN, ALGO_INDEX, ALGO_SIG, ALGO_STREAM, BANDING_CPU, BANDING_CUDA, CRIT_HLL_A, CRIT_HLL_A_SMH_A,  # noqa: F401
                   CRIT_HLL_AN, CRIT_NONE, CRIT_SMH_A, CRIT_SMH_C, ESTIMATOR_HLL, ESTIMATOR_SMH, F32, F64, FP_FMA, FP_STRICT, MEASURE_CONTAINMENT, MEASURE_INTERSECTION, MEASURE_JACCARD, MEASURE_MAX_CONTAINMENT, MEASURE_SMH_JACCARD, MEASURE_SMH_MATCHES, MEASURE_UNION, MODE_CB_SMH, MODE_SMH, REP_MAX_DEGREE, REP_MAX_RANK, REP_MIN_RANK, REP_PRIORITY, MERGE_SEGMENT, TOPK_MAX, TOPK_ROUNDS_AUTO, SelhipError, hip_lib, host_lib)
from .selection import (PAIR_DTYPE, Selector, banding, cluster_from_filelist, components, greedy_from_filelist, greedy_representatives, spanning_forest, forest_cluster_counts, forest_cut, forest_linkage, forest_table, forest_from_filelist, order_code, rep_code, format_lines, hll_fold, merge_sketches, selector_from_rows, merge_from_filelist, read_groups, write_merged, cluster_names, load_dataset, matrix_from_filelist, measure_code, estimator_code, smh_value, min_matches, containment_matches, ooc_select,  # noqa: F401
                        query_from_filelists, query_matrix_from_filelists,
                        read_pair_list, read_results, select_from_filelist, select_pairs_from_filelist, sort_by_card, write_results)
from .synth import SYNTH_CONFIGS, SynthConfig, harden, stream_model, synth_device, synth_host  # noqa: F401

__all__ = ["Selector", "components", "cluster_from_filelist", "rep_code", "REP_MAX_DEGREE", "REP_MIN_RANK", "REP_MAX_RANK", "REP_PRIORITY", "greedy_representatives", "greedy_from_filelist", "spanning_forest", "forest_cluster_counts", "forest_cut", "forest_linkage", "forest_table", "forest_from_filelist", "order_code", "min_matches", "containment_matches", "CRIT_SMH_A", "CRIT_HLL_A", "CRIT_HLL_AN", "CRIT_HLL_A_SMH_A", "CRIT_NONE", "CRIT_SMH_C", "matrix_from_filelist", "query_matrix_from_filelists", "MEASURE_JACCARD", "MEASURE_UNION", "MEASURE_SMH_MATCHES", "MEASURE_SMH_JACCARD", "MEASURE_INTERSECTION", "MEASURE_CONTAINMENT", "MEASURE_MAX_CONTAINMENT", "measure_code", "ESTIMATOR_HLL", "ESTIMATOR_SMH", "estimator_code", "smh_value", "F64", "F32", "ooc_select", "query_from_filelists", "write_results", "read_results", "banding", "select_from_filelist", "select_pairs_from_filelist", "read_pair_list", "load_dataset", "sort_by_card", "format_lines", "hll_fold", "merge_sketches", "selector_from_rows", "merge_from_filelist", "read_groups", "write_merged", "cluster_names", "MERGE_SEGMENT",
           "SynthConfig", "SYNTH_CONFIGS", "synth_device", "synth_host", "harden", "stream_model", "hip_lib", "host_lib", "SelhipError",
           "MODE_SMH", "MODE_CB_SMH", "ALGO_AUTO", "ALGO_STREAM", "ALGO_SIG", "ALGO_HASHJOIN", "ALGO_INDEX", "FP_FMA", "FP_STRICT", "PAIR_DTYPE", "TOPK_MAX", "TOPK_ROUNDS_AUTO"]

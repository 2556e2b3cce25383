// selection_kernels.hip -- gfx950 (MI355X, CDNA4, wave64) kernels and the C ABI of libselhip.so.
//
// Replaces, for the all-pairs sketch-selection path of sanhue903/CUDA_Selection_Criteria:
//   src/selection_kernels.cu:13-177 (kernel_smh, kernel_CBsmh, launchers)
//   include/criteria_sketch_cuda.cuh:11-65 (device CB / smh_a / hll_union_card)
// with the RESULT SEMANTICS of the CPU path src/selection.cpp:270-291 (see include/selection_hip.h).
//
// This is the kernel translation unit of the library: it only includes.  The kernels live in the kernel_*.cuh headers (all integer
// except the estimator; no MFMA), the host side in host_plan.hpp (decisions), host_context.hpp (context), host_pass.hpp (pass scheduler) and abi_*.inc (C ABI);
// the multi-GPU and out-of-core drivers are translation units of their own (selhip_multi.hip, selhip_ooc.hip):
//   pair_value.hpp      selhip::pair_value: what a pair's value is under J, the intersection estimate and the two containments -- the one
//                       definition that stage 2 (kernel_hll.cuh, kernel_dense.cuh) and kernel_matrix.cuh call
//   common.cuh          launch constants, per-pass counters, WaveAppender / block_append (LDS-staged appends, one atomic per flush)
//   kernel_bounds.cuh   cb_bounds_kernel      e_i = (size_t)card_i, CB cut-off hi(i), first non-zero rank
//   kernel_verify.cuh   smh_a_lane (the literal predicate), sig_candidate_ok (the one statement of "signature equal, band not equal"),
//                       verify16_batch (16 lanes per pair), verify_kernel / verify16_kernel: the exact verification behind ALGO_SIG
//   kernel_stream.cuh   smh_stream_kernel     stage 1 ALGO_STREAM: query tile in LDS/VGPRs, candidates streamed row-major,
//                                             v_cmp_eq_u64 lane masks folded on the scalar unit; smh_generic_kernel
//   kernel_smhc.cuh     smh_count_kernel      stage 1 of criterion smh_c: at least c_min equal buckets -- the stream kernel's enumeration with a
//                                             count (v_cmp_eq_u64, s_bcnt1, scalar adds, one compare) in place of the band fold, over the
//                                             triangle or a query rectangle; smh_count_generic_kernel for every other m
//   kernel_sigjoin.cuh  sig_build / sig_join   stage 1 ALGO_SIG: all-pairs band-signature join (DPP broadcast), hash join
//   kernel_hll.cuh      hll_union_hist_kernel, ertl_select_kernel (stage 2), enum_pairs / aux_fused (hll_a, hll_an)
//   kernel_hllbs.cuh    hll_bitslice_kernel, hll_union_hist_bs_kernel: stage 2a on bit-sliced registers (bit-serial max, decode tree, v_bcnt)
//   kernel_pairlist.cuh explicit pair lists (test building blocks)
//   kernel_pairs.cuh    stage 1 of the pair-list passes (a caller's list of pairs under any criterion) and of the drop-in launchers'
//                       explicit-list path: filter, signature verification, direct band comparison
//   kernel_sketch.cuh   synth_kernel, sketch_build_kernel (build_sketch on the GPU), sketch_build_items_kernel / sketch_split_finish_kernel
//                       (the same sketches with long genomes split across workgroups), permute_rows
//   kernel_small.cuh    small_pass_kernel: the whole pass of a set of <= 2 048 genomes in one cooperative launch
//   kernel_query.cuh    query passes (a query set against the database): CB windows, rectangular signature join, verification,
//                       literal stream kernel for any band shape, stage 2a on two sets' bit planes
//   kernel_query_index.cuh ALGO_INDEX of the query passes: the database's band signatures sorted per band (built once, kept), one
//                       binary search per (query, band) in place of the rectangular join
//   kernel_dense.cuh    dense_select_kernel: criterion "none" -- every pair of the (CB-pruned) pair space to the Jaccard test, union
//                       histograms into an LDS tile and the estimator in one launch
//   kernel_matrix.cuh   matrix_kernel: the union size, the Jaccard estimate, the intersection estimate or a containment of every pair as a dense array (the middle of
//                       dense_select_kernel over a rectangle, typed and mirrored stores; selhip_ctx_matrix / _query_matrix)
//   kernel_matrix_smh.cuh  matrix_smh_kernel / matrix_smh_generic_kernel: the SuperMinHash bucket-match count, or count / m, of every
//                       pair as a dense array (query rows in VGPRs, candidate rows streamed past them; the same entry points)
//   kernel_topk.cuh     top-k of a pass: records grouped by owner (count, scan, scatter) -- a query pass's by query, an all-pairs
//                       pass's for both of their genomes --, radix select of each owner's K best, bitonic sort of the winners
//   kernel_query_aux.cuh the auxiliary-HLL criteria of query passes: hll_a / hll_an over each query's CB window, the hll_a stage
//                       of hll_a + smh_a over the smh_a survivors
//   hll_fold.hpp        selhip::fold_contrib / fold_combine: how a register of precision p folds into the sketch of a lower precision
//                       (shared with libselhost.so, like ertl_mle.hpp)
//   kernel_fold.cuh     hll_fold_kernel: the auxiliary HLL sketches folded from the main registers, one streaming read (in a lane, across
//                       the lanes of a load, across the loads of a wave)
//   kernel_graph.cuh    what the three graph kernels below share: the lock-free union-find with parent[x] <= x, the wave-aggregated degree
//                       tally, the three kinds of edge list, the range check of an entry with its tally, the order-preserving image of a value
//   kernel_cluster.cuh  single-linkage clusters of a record list: the union-find of kernel_graph.cuh (agent-scope atomic minima,
//                       one lane per record), flattened labels, dense ids, degrees, sizes and one representative per cluster
//   kernel_greedy.cuh   greedy representative clusters of a record list (CD-HIT / UCLUST): the first maximal independent set under a key
//                       order in rounds of one edge and one vertex launch, then every member to its most similar representative
//   kernel_forest.cuh   maximum spanning forest of a record list, its single-linkage dendrogram: Boruvka rounds of two record launches (best
//                       value, then smallest pair among the equal), a hook and a flatten launch over the union-find of kernel_graph.cuh
//   kernel_linkage.cuh  agglomerative hierarchy of a dense f64 distance matrix (single, complete, average, weighted linkage): rounds of
//                       reciprocal nearest neighbours -- row scans of the dirty rows, ordered pair compaction, Lance-Williams update in place
//   kernel_merge.cuh    sketches merged by group: a counting sort of the members, then a segmented reduction of the rows (u8 maximum of the
//                       HLL registers, u64 minimum of the SuperMinHash buckets) in segments of at most SELHIP_MERGE_SEGMENT members per level
//
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off (see csrc/Makefile).
#include <hip/hip_runtime.h>
#include <rocprim/device/device_scan.hpp>         // exclusive scan of the per-row survivor counts (grouping for stage 2)
#include <rocprim/iterator/transform_iterator.hpp> // the top-k scan reads the per-query counts packed on the fly
#include <rocprim/device/device_merge_sort.hpp>   // the spanning forest's edges into their order: a comparison sort of 16-byte records
#include <rocprim/device/device_radix_sort.hpp>   // ALGO_HASHJOIN and the query index: the key sort is a library call, everything else is hand-written

#include <algorithm>
#include <type_traits>
#include <array>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <mutex>
#include <string>
#include <tuple>
#include <vector>

#include "../../include/selection_hip.h"
#include "selhip_internal.h"
#include "ertl_mle.hpp"
#include "pair_value.hpp"      // the value of a pair under every HLL measure (J, intersection, containments): one definition
#include "synth.hpp"
#include "hll_fold.hpp"        // how a main HLL register folds into the auxiliary sketch of a lower precision: one definition

#include "common.cuh"
#include "kernel_bounds.cuh"
#include "kernel_verify.cuh"
#include "kernel_stream.cuh"
#include "kernel_smhc.cuh"
#include "kernel_sigjoin.cuh"
#include "kernel_hll.cuh"
#include "kernel_hllbs.cuh"
#include "kernel_pairlist.cuh"
#include "kernel_pairs.cuh"
#include "kernel_sketch.cuh"
#include "kernel_small.cuh"
#include "kernel_query.cuh"
#include "kernel_query_aux.cuh"
#include "kernel_query_index.cuh"
#include "kernel_dense.cuh"
#include "kernel_topk.cuh"
#include "kernel_fold.cuh"
#include "kernel_graph.cuh"      // (in front of the three graph kernels: union-find, edge lists, range check, value image)
#include "kernel_cluster.cuh"
#include "kernel_greedy.cuh"
#include "kernel_forest.cuh"
#include "kernel_linkage.cuh"     // (behind kernel_forest.cuh: ClusterBad, ForestEdge)
#include "kernel_merge.cuh"

#include "host_plan.hpp"         // host decisions that are plain arithmetic: build shape, pass plan, criterion constants, overflow rule
#include "kernel_matrix.cuh"     // (behind host_plan.hpp: the kernel reads the unit, slab and mirror rules written there)
#include "kernel_matrix_smh.cuh" // (behind kernel_matrix.cuh: MatrixOut)
#include "host_context.hpp"      // struct selhip_ctx, device buffers (signature sets, bit planes, counter sets), timers, helpers
#include "host_pass.hpp"         // pass scheduler: dispatch of every stage, chunk lanes, scratch sizing
#include "host_pairs.hpp"        // pair-list passes: the chain behind selhip_ctx_run_pairs
#include "host_query.hpp"        // query passes: Q x D (windows, signature join or stream, verification, stage 2)
#include "host_topk.hpp"         // top-k of a query pass and of an all-pairs pass: scratch, launches, the count the result accessors expose
#include "host_graph.hpp"        // the graph calls' shared front end: admission, the run of an admitted call, reports, the block carver
#include "host_cluster.hpp"      // single-linkage clusters: grids and launches behind selhip_ctx_cluster / selhip_components
#include "host_greedy.hpp"       // greedy representative clusters: rounds and launches behind selhip_ctx_cluster_greedy / selhip_greedy_representatives
#include "host_forest.hpp"       // maximum spanning forest: rounds, sort and launches behind selhip_ctx_spanning_forest / selhip_spanning_forest
#include "host_linkage.hpp"      // dense-matrix hierarchy: checks, scratch and rounds behind selhip_linkage / selhip_ctx_linkage
#include "host_merge.hpp"       // sketches merged by group: checks, levels and launches behind selhip_merge_sketches / selhip_ctx_merge_groups
#include "host_build.hpp"       // split sketch builder: items, launches, the reduction through merge_run, the fallback launch
#include "abi_context.inc"       // C ABI: context (create, upload / attach, run, results, timing)
#include "abi_pairs.inc"         // C ABI: pair-list passes (run_pairs)
#include "abi_query.inc"         // C ABI: query passes (upload / attach queries, run_queries)
#include "abi_matrix.inc"        // C ABI: dense matrices (matrix, query_matrix)
#include "abi_cluster.inc"       // C ABI: clusters of the result list (cluster) and of a caller's edge list (components)
#include "abi_greedy.inc"        // C ABI: greedy representative clusters of the result list (cluster_greedy) and of a caller's edge list (greedy_representatives)
#include "abi_forest.inc"        // C ABI: maximum spanning forest of the result list (ctx_spanning_forest) and of a caller's edge list (spanning_forest)
#include "abi_linkage.inc"       // C ABI: average / complete / weighted / single linkage of a dense matrix (ctx_linkage, linkage)
#include "abi_merge.inc"        // C ABI: sketches merged by group (merge_sketches, ctx_merge_groups)
#include "abi_build.inc"        // C ABI: sketch construction with long genomes split across workgroups (build_sketches_split, build_split_plan)
#include "abi_blocks.inc"        // C ABI: building blocks, synthetic sketches, sketch construction, memory helpers
#include "abi_compat.inc"        // C ABI: drop-in launch_kernel_smh / launch_kernel_CBsmh

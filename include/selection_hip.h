/*
 * selection_hip.h -- C ABI of libselhip.so: the MI355X (gfx950) replacement for the reference's GPU
 * kernel boundary of the all-pairs sketch-selection step.
 *
 * What it replaces in sanhue903/CUDA_Selection_Criteria (paths relative to that repository):
 *   src/selection_kernels_wrapper.hpp:6-45   struct Result, launch_kernel_smh, launch_kernel_CBsmh
 *   src/selection_kernels.cu:13-177          kernel_smh / kernel_CBsmh and their launchers
 *   include/criteria_sketch_cuda.cuh:11-65   device CB / smh_a / hll_union_card
 *   src/selection_cuda.cpp:152-182           the raw cudaMalloc/cudaMemcpy/launch/copy-back sequence
 *                                            (here: the selhip_ctx_* lifecycle)
 *
 * RESULT SEMANTICS are those of the reference's CPU path src/selection.cpp:270-291 (the parity target
 * named by BASELINE.json), NOT of its CUDA kernels (which use a different HLL estimator, never apply
 * CB and index out of bounds -- SURVEY.md section 2.3):
 *   pair (i,k), i<k in ascending-cardinality rank order, is selected iff
 *     e_k != 0                                   (selection.cpp:281; e = (size_t)cardinality, :275,:280)
 *     [CB modes]  (double)e_i / (double)e_k >= (double)tau_f            (criteria_sketch.hpp:45-49)
 *     smh_a: some band of n_rows consecutive u64 buckets is entirely equal   (criteria_sketch.hpp:66-81)
 *     J = ((double)e_i + (double)e_k - U) / U >= (double)tau_f, U = Ertl-MLE estimate of the register-wise
 *         max of the two p=14 HyperLogLog sketches                     (hll.h:1188-1210 -> :629-688)
 *
 * All functions return 0 on success or a negative SELHIP_E_* code; nothing throws across the ABI.
 * No HIP, torch or C++ types appear in any signature.  Pointers named d_* are DEVICE pointers owned by
 * the caller (hipMalloc, or a torch tensor's data_ptr()); h_* are host pointers.
 */
#ifndef SELECTION_HIP_H
#define SELECTION_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SELHIP_OK              0
#define SELHIP_E_BADARG       -1   /* null pointer, bad size, rows*bands != m, ...                      */
#define SELHIP_E_HIP          -2   /* a HIP runtime call failed; see selhip_last_error()                */
#define SELHIP_E_OVERFLOW     -3   /* an output buffer was too small; nothing was lost: counts are exact */
#define SELHIP_E_NODEVICE     -4   /* no usable gfx950 device                                           */
#define SELHIP_E_STATE        -5   /* call sequence error (e.g. run before upload)                      */
#define SELHIP_E_NOMEM        -6   /* the call would need more device scratch than it may take          */

/* == struct Result of src/selection_kernels_wrapper.hpp:6-9 (same layout: 12 bytes) */
typedef struct { int32_t x, y; float sim; } selhip_result_t;
/* == CUDA int2 used for the pair list (wrapper.hpp:16) */
typedef struct { int32_t x, y; } selhip_int2_t;
/* full-precision output record of the context API: the CPU path prints J with std::to_string(double) */
/* (`jaccard` carries the value of the pass's MEASURE: J by default, the max containment after selhip_ctx_set_measure) */
typedef struct { int32_t i, k; double jaccard; } selhip_pair_t;

/* modes, after the two timed regions of experiments/src/time_smh.cpp:229-257 / :261-292 */
#define SELHIP_MODE_SMH      0     /* "smh_a": every pair i<k (e_k==0 skipped), no CB                    */
#define SELHIP_MODE_CB_SMH   1     /* "CB+smh_a": = src/selection.cpp:270-291                            */

/* stage-1 algorithm */
#define SELHIP_ALGO_AUTO     0
#define SELHIP_ALGO_STREAM   1     /* full m-bucket compare, candidates streamed row-major, query tile in LDS */
#define SELHIP_ALGO_SIG      2     /* 32-bit band signatures joined all-pairs, exact verify of candidates  */
#define SELHIP_ALGO_HASHJOIN 3     /* sub-quadratic: (band, signature) keys radix-sorted, candidates read off the runs of equal
                                      keys, exact verify -- same survivors, but pairs are no longer compared one by one
                                      (never chosen by AUTO; not what the pair-comparisons/s metric measures)          */
#define SELHIP_ALGO_INDEX    4     /* query passes only (section 2b): the database's band signatures sorted per band, built once and
                                      kept; a pass is one binary search per (query, band) plus the matches -- the records and
                                      statistics of SIG (never chosen by AUTO; every other entry answers "bad algo 4")   */

/* selection criterion applied before the final HLL-14 Jaccard test (src/selection.cpp -c ...):
 *   SMH_A        src/selection.cpp:228-291   (the north_star path)
 *   HLL_A        src/selection.cpp:122-173   auxiliary HLL p = ctz(aux_bytes), criteria_sketch.hpp:36-43,60-64
 *   HLL_AN       src/selection.cpp:175-227   criteria_sketch.hpp:22-34,52-58 (order_n = 1, Z = 1.96)
 *   HLL_A_SMH_A  both hll_a and smh_a must select the pair (BASELINE.json config 5: "hll_a prefilter +
 *                smh_a two-stage criterion"); evaluated smh_a first, hll_a on its survivors -- the selected
 *                set is the intersection either way
 *   NONE         no criterion at all: every pair that e_k != 0 and (in SELHIP_MODE_CB_SMH) the CB bound leave goes to the
 *                Jaccard test -- src/selection.cpp:270-291 with the smh_a test removed.  SELHIP_MODE_CB_SMH gives the reference
 *                README's "CB criterion" line, SELHIP_MODE_SMH its "no criterion (baseline case)": the ground truth the other
 *                criteria are lossy filters of.  A pair that another criterion selects is selected here with the same record
 *                (same i, k, J bits): result(c) is a subset of result(NONE) for every c, same mode, tau_f and FP flavour.
 *                Needs p_hll = 14 (SELHIP_E_BADARG otherwise); reads neither the SuperMinHash nor the auxiliary HLL sketches */
#define SELHIP_CRIT_SMH_A        0
#define SELHIP_CRIT_HLL_A        1
#define SELHIP_CRIT_HLL_AN       2
#define SELHIP_CRIT_HLL_A_SMH_A  3
#define SELHIP_CRIT_NONE         4
/* smh_c: at least c_min of the m SuperMinHash buckets equal (selhip_ctx_set_min_matches), i.e. the SuperMinHash Jaccard estimate
 * c / m >= c_min / m -- exhaustive over the pass's pair space, no banding loss; n_rows, n_bands and algo are ignored */
#define SELHIP_CRIT_SMH_C        5

/* estimator arithmetic flavour (see csrc/ertl_mle.hpp) */
#define SELHIP_FP_FMA        1     /* = reference built by its Makefile on an FMA-capable x86 host (default) */
#define SELHIP_FP_STRICT     0     /* = reference built with -ffp-contract=off                              */

/* ---------------------------------------------------------------------------------------------------
 * 1. Drop-in launchers: same names and parameter lists as src/selection_kernels_wrapper.hpp:11-45
 *    (CUDA int2 -> selhip_int2_t, Result -> selhip_result_t, void -> int status).
 *    All pointers are device pointers; out must hold total_pairs records (reference contract,
 *    selection_cuda.cpp:164); *out_count is zeroed by the launcher (selection_kernels.cu:137,166).
 *    pairs == NULL selects the IMPLICIT triangle i < k < n of the reference driver (selection_cuda.cpp:146-150) without
 *    materialising the 8 B/pair list: total_pairs must then be n(n-1)/2, which fixes n; cards must be ascending (the
 *    driver's order); this variant runs the all-pairs path of the context API and returns after the pass.
 *    With an explicit list the launchers are asynchronous on the null stream, like the reference.
 *    An explicit list is taken ENTRY BY ENTRY, in the orientation listed, as the reference's kernels take it: an entry {x, y} is
 *    evaluated iff (size_t)cards[y] != 0 and, for launch_kernel_CBsmh, (double)(size_t)cards[x] / (double)(size_t)cards[y] >= tau
 *    -- x's cardinality over y's, whichever is larger, so a reversed entry {larger, smaller} has a ratio >= 1 and is never cut, and an
 *    entry whose x is an empty sketch is cut at any tau > 0 --; an evaluated entry with an equal band whose J reaches tau gives the
 *    record {x, y, (float)J} with x and y as listed, once per occurrence of the entry.  Nothing is deduplicated and cards need not
 *    be ascending.  x == y is no special case: such an entry has every band equal and J = (2 e - t) / t with t the estimate of the
 *    sketch's own register row.  No rank is checked (the parameter list carries no genome count): a rank outside the arrays is
 *    the caller's error and reads out of bounds.
 *    m_aux is the number of u64 buckets per sketch, m_hll the number of HLL registers (16384).
 *    launch_kernel_smh evaluates every listed pair; launch_kernel_CBsmh additionally applies CB
 *    (the reference kernel of that name does not, selection_kernels.cu:63-117 -- documented defect).
 *    blockSize is accepted and ignored (the kernels choose their own wave64 geometry).
 *    launch_kernel_smh64 / launch_kernel_CBsmh64: the same with int64_t total_pairs and a 64-bit *out_count -- the
 *    reference's `int total_pairs` / `int idx` (selection_kernels.cu:29-30) overflow beyond 2^31 pairs (n > 65 536).
 * --------------------------------------------------------------------------------------------------- */
int launch_kernel_smh(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                      const selhip_int2_t* pairs, int total_pairs, double tau,
                      int m_aux, int m_hll, int n_rows, int n_bands,
                      selhip_result_t* out, int* out_count, int blockSize);
int launch_kernel_CBsmh(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                        const selhip_int2_t* pairs, int total_pairs, double tau,
                        int m_aux, int m_hll, int n_rows, int n_bands,
                        selhip_result_t* out, int* out_count, int blockSize);
int launch_kernel_smh64(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                        const selhip_int2_t* pairs, int64_t total_pairs, double tau,
                        int m_aux, int m_hll, int n_rows, int n_bands,
                        selhip_result_t* out, int64_t* out_count, int blockSize);
int launch_kernel_CBsmh64(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                          const selhip_int2_t* pairs, int64_t total_pairs, double tau,
                          int m_aux, int m_hll, int n_rows, int n_bands,
                          selhip_result_t* out, int64_t* out_count, int blockSize);

/* ---------------------------------------------------------------------------------------------------
 * 2. Context API: owns the derived device buffers (truncated cards, CB bounds, band signatures,
 *    candidate / result lists) that selection_cuda.cpp:152-182 handles with raw CUDA calls.
 * --------------------------------------------------------------------------------------------------- */
typedef struct selhip_ctx selhip_ctx;

int  selhip_device_count(void);
int  selhip_ctx_create(selhip_ctx** out, int device);
void selhip_ctx_destroy(selhip_ctx* ctx);
/* message of the last failure on this context (never NULL); ctx may be NULL for creation errors */
const char* selhip_last_error(const selhip_ctx* ctx);
/* Host threads.  DIFFERENT contexts may be used from different host threads at the same time, on the same device or on different
 * ones, and so may the entries that take no context (sections 1, 3, 4, 4b): every context, and every call of a context-free entry,
 * owns its scratch, its counters and its cached products; nothing of them is shared.  selhip_ooc_select (up to four worker threads on
 * one device) and selhip_multi_select (one thread per device) rest on this.  ONE context is used by one thread at a time: its calls
 * are not locked against each other, and the caller orders them (it may hand a context from thread to thread).
 * selhip_last_error(NULL) is per thread: the message of the last failure of a call made ON THE CALLING THREAD (any context, or none);
 * selhip_last_error(ctx) is the context's own message, whichever thread reads it.  The two settings that are process-wide are the test
 * hooks "cluster_blocks" and "vertex_blocks" of selhip_ctx_set_param (the grids of the kernels that take a lane per record, and per
 * vertex, row or slot; 0 = sized from the input): each is set through any context, holds for every graph call of the process (sections
 * 2g, 2h, 2j, 2k and their context-free forms in section 3; "vertex_blocks" also for the merge by group), may be set while other
 * threads work, is read back by selhip_ctx_get_param, and changes no answer.  Calls that free
 * device memory (below) wait for the whole device and so for the other threads' work; they delay it and do not disturb it.
 * tests/test_threads_gpu.py runs every entry from several threads at once. */

/* Run all work of this context on `hip_stream` (a hipStream_t passed as void*; NULL = null stream).
 * This holds on a NON-BLOCKING stream (hipStreamNonBlocking, e.g. a torch pool stream), which the null stream does not wait for:
 * every launch, memset, copy and sort of every entry of sections 2 - 2h goes to the stream, the second chunk lane of a pass
 * (selhip_ctx_set_pipeline) starts behind an event of the stream and is joined by another, and state a context keeps (signature
 * cache, query index, counter sets) is complete before selhip_ctx_set_stream returns with another stream.  A call on a context whose
 * buffers are sized neither touches the null stream nor waits for the device (tests/test_streams_gpu.py runs every entry beside a
 * blocked null stream).  What DOES wait for the whole device is a call that frees device memory (hipFree): a pass that outgrows one
 * of its lists and repeats; the first SELHIP_ALGO_INDEX pass behind an upload / attach of the database, whose sort scratch goes away
 * when the index stands; any buffer that grows; and, in section 3, selhip_hll_bitslice, selhip_hll_union_hist_planes,
 * selhip_components, selhip_greedy_representatives, selhip_spanning_forest and selhip_linkage, whose scratch lives for the call
 * (selhip_ctx_linkage too: its n * n cells of scratch are taken and released in every call). */
int selhip_ctx_set_stream(selhip_ctx* ctx, void* hip_stream);
/* Chunk lanes of a pass (smh_a / hll_a+smh_a): the query rows are cut into `chunks` equal-pair chunks and every chunk runs its
 * whole chain (join, verify, [auxiliary criterion], grouping, HLL union histograms, estimate) on one of two internal streams
 * (the context's own and one more), so that one chunk's short tail kernels run beside the other chunk's join.
 * -1 = automatic (the default: 2 chunks from 5e8 pairs per pass with the signature join, else 1), 0 / 1 = off, 2..8 = chunk
 * count.  Results and counters do not depend on it.  (Round 1's stage-1-stream / stage-2-stream pipeline was replaced.) */
int selhip_ctx_set_pipeline(selhip_ctx* ctx, int chunks);
/* Row interleave for sharding a pass over several devices/ranks: the rows [row_begin, row_end) of the following runs are
 * cut into blocks of block_rows rows (a multiple of 32), dealt boustrophedon: of the n_parts blocks of cycle q the run evaluates
 * block number `part` when q is even and block number n_parts - 1 - part when q is odd (rows get shorter towards the end of the
 * triangle, so a plain round-robin deal would give part 0 the longest row block of every cycle).  Every rank then gets the
 * same share of the pair space AND of the survivors, whatever the triangle's shape (a contiguous equal-pair cut hands the
 * last of 8 ranks ~35 % of all rows, i.e. of all stage-2 work).  n_parts <= 1 switches it off. */
int selhip_ctx_set_row_interleave(selhip_ctx* ctx, int block_rows, int n_parts, int part);
/* Rectangular passes: the following runs only take candidates k >= k_min (in addition to k > i), i.e. rows [row_begin,
 * row_end) x columns [k_min, n).  With the uploaded array = block I followed by block J of a larger sorted set,
 * rows [0, |I|) and k_min = |I| evaluates exactly the pairs I x J (the out-of-core driver below).  Reset to 0 by upload/attach. */
int selhip_ctx_set_candidate_begin(selhip_ctx* ctx, int64_t k_min);
/* Tunables (integers by name; results never depend on them):
 *   "join_q"      query side of the 16-bit signature join: 1 (default) = tile of query rows staged in LDS, broadcast LDS reads
 *                 (sigl_join_kernel); 0 = DPP row broadcast from registers (sig16_join_kernel, the round-1 form)
 *   "join_qt"     query rows per block of the signature join: 0 (default) = automatic (32 below 1e8 pairs per pass, 64 below 4.5e8, 128
 *                 beyond), or a multiple of 16
 *   "join_bits"   16 (default): all-pairs join on 16-bit band signatures packed two per dword, its matches cut back to the
 *                 32-bit candidate set during verification; 15: the same with 15-bit signatures and flag arithmetic made of
 *                 plain VOP2 instructions only (LDS form); 32: join on the 32-bit signatures directly
 *   "join_form"   inner loop of the 16-bit LDS-tile join: 2 (default) = bit-sliced signatures (plane j of a genome = bit 16 + j of
 *                 every band's signature), one v_bitop3_b32 per dword -- for band shapes of the tiled signature build (power-of-two m,
 *                 2 <= rows per band <= 32, "sig_tile" = 1), the packed form 0 otherwise; 0 = packed dwords, v_xor_b32 + v_pk_min_u16;
 *                 1 = zero-half test on the packed dwords (v_xor_b32, v_sub_u32, v_bitop3_b32; measured slower)
 *   "join_t"      sliced join: groups of 64 candidates per wave, 1 or 2 (at most 64 bands; 1 beyond); 0 (default) = automatic (2 from
 *                 4.5e8 pairs per pass)
 *   "join_tri"    1: the LDS-tile join launches only the (tile, candidate block) units above the diagonal (contiguous rows; measured:
 *                 no gain); 0 (default): the rectangle, whose blocks under the diagonal leave at once
 *   "join_db"     1 (default) / 0: double-buffered query batches in the DPP form of the 16-bit join
 *   "join_wpb"    waves per block of the 16-bit join: LDS form 4 (default) or 8, DPP form 1 or 4
 *   "sig_tile"    1 (default): signature build 16 genomes per block with an LDS transpose; 0: one thread per bucket
 *   "sig_cache"   1: the band signatures are kept across the passes of this context (they depend on the sketches and the band shape
 *                 only; upload / attach drop them) -- for callers that run many passes over one set, e.g. every rank of a
 *                 strong-scaled job; 0 (default): every pass builds them
 *   "hist_algo"   stage 2a: -1 (default) / 1 = on the registers' bit planes, written at upload / attach (hll_union_hist_bs_kernel:
 *                 bit-serial max, decode tree, population counts; p = 14 only); 0 = on the byte rows with a lane-private LDS
 *                 histogram (hll_union_hist_runs_kernel).  Takes effect at the next upload / attach.
 *   "hist_run"    pairs a wave of stage 2a takes at a time (0 = automatic: 4 on a grouped list; the byte-row kernel: 1, or 4 with the label order);
 *                 the bit-plane kernel takes at most 64;
 *   "hist_dense_degree"  bit-plane kernel on a grouped list: from this many survivors per query row of the pass (default 32; 0 = always, -1 = never) every
 *                 XCD walks the whole list and takes the pairs whose candidate row hashes to it, so that its L2 keeps an eighth of the
 *                 candidate rows instead of streaming all of them (a dense survivor graph; bench.py --hard: 6.2 -> 1.5 GB per pass from beyond L2,
 *                 DESIGN.md section 4.3);
 *   "hist_blocks" one-wave blocks of the byte-row kernel, "hist_bs_blocks" four-wave blocks of the bit-plane kernel (multiples of 8);
 *   "hist_sparse" 1: the all-pairs bit-plane kernel decodes only the values below the set's sparse threshold T from the planes and
 *                 takes every register >= T from sorted per-genome lists written with the planes (T = the smallest multiple of 4 at which
 *                 every genome holds at most 128 such registers; none above 24); 0: every value from the planes; -1 (default): 1 for sets
 *                 whose bit planes take at most 192 MiB, and for larger ones where T <= 12 (stage 2a then reads a four-plane image of
 *                 min(register, 15), 8 KiB per genome, written with the lists), else 0.  Same counts either way;
 *                 selhip_ctx_get_param "hist_sparse_t" reports the T in use (0 = off).  Query passes and the one-launch small pass
 *                 always decode every value from the planes;
 *   "small_pass"  -1 (default) / 1: a set of up to 2 048 genomes with criterion smh_a takes its whole pass in ONE launch
 *                 (small_pass_kernel: bounds + signatures, a grid barrier, then join, verification, union histograms and estimator
 *                 inside each block; the barrier's wait is bounded and a pass that runs out of patience is repeated on the regular path);
 *                 2: the same through hipLaunchCooperativeKernel (+15 us per launch); 0: the regular chain of launches
 *   "group_min_n" sets of up to this many genomes (default 2 048) skip the stage-2 grouping: two latency-bound launches that buy nothing
 *                 while the whole table stays in cache; 0 = group always
 *   "group_label" stage-2 grouping lays the query-row buckets out by label = a row's smallest partner, so that the pairs of a
 *                 cluster of similar genomes are neighbours in the list and their HLL rows stay in L2 (-1 = automatic: sets
 *                 whose HLL rows exceed 192 MiB and passes of >= 4e8 pairs; 0 off; 1 on);
 *   "dense_fused" SELHIP_CRIT_NONE: 1 (default) the pass is ONE kernel behind the bounds (dense_select_kernel: union histograms into an
 *                 LDS tile, estimator and J test in the same wave); 0 the list route -- the pair space listed explicitly in row
 *                 sub-passes, then the union-histogram and estimator kernels of the other criteria.  Same records and statistics;
 *   "matrix_mirror" a MEASUREMENT switch of the dense matrices (section 2f), the one name here that changes what is written: 1 (default) a
 *                 self matrix stores every computed cell (i, k), i < k < r1, at (k, i) as well; 0 it stores no mirrored cell, so a call
 *                 writes only the columns [0, r0) and [i, n) of each row i of its slab [r0, r1) and the matrix is INCOMPLETE below the
 *                 diagonal -- for timing the mirrored stores (scripts/bench_matrix.py), not for use.  selhip_ctx_get_param reads it back;
 *   "timed_kernel" see selhip_ctx_timing.
 * (The library also answers to a few names that are NOT part of this interface -- hooks of its own test-suite and measurement
 * knobs, listed at selhip_ctx_set_param in csrc/selection_kernels.hip.) */
int selhip_ctx_set_param(selhip_ctx* ctx, const char* name, int value);
/* what the context decided (read-only): "hll_khi" (largest p = 14 register value + 1; 0 = no bit planes), "hist_bitplanes",
 * "label_order", "join_tile_rows", "join_form_used" (kernel form of the last LDS-tile join: 0 packed minimum, 1 15-bit, 2 zero-half,
 * 3 bit-sliced; -1 none or the DPP join), "chunks" (chunk lanes of the last pass), "small_pass_used" (the last pass was the one-launch small pass),
 * "query_db_sig_builds" (builds of the database's band signatures by query passes since the database was loaded, section 2b),
 * "query_db_index_builds" (builds of SELHIP_ALGO_INDEX's sorted signature index since the database was loaded, section 2b),
 * "query_db_index_kib" (resident size of that index in KiB, 0 = none held),
 * "hist_sparse_t" (the sparse threshold the all-pairs stage 2a uses, 0 = every value from the bit planes),
 * "dense_route_used" (SELHIP_CRIT_NONE: the route of the last such pass, 1 = the fused kernel, 0 = the list route; -1 = none yet),
 * "query_topk", "query_topk_lds_cap" (top-k of the query passes, section 2b),
 * "allpairs_topk" (the current k of selhip_ctx_set_allpairs_topk, 0 = off),
 * "pairs_route_used" (stage 1 of the last pair-list pass, section 2e),
 * "pairs_gpw" and "pairs_grid" (the launch shape of that stage 1: the groups of four entries a wave of the direct route or of the
 * smh_c count takes per batch, 1 .. 16 by the list's length -- 0 for the kernels of one lane per entry, the signature route and the
 * criteria without an smh_a stage -- and the kernel's blocks, of the first window where the list goes in windows; both 0 after an
 * empty list, -1 = no list pass yet),
 * "matrix_smh_path_used" (the kernel of the last matrix call with a SuperMinHash measure, section 2f: 1 = the register-tile kernel
 * of m = 128, 256, 512 or 1024 buckets, 0 = the generic kernel of every other m; -1 = none yet),
 * "clusters_last" (the number of clusters the last selhip_ctx_cluster call found, section 2g; -1 = none yet),
 * "greedy_clusters_last" and "greedy_rounds_last" (the clusters the last selhip_ctx_cluster_greedy call found and the rounds its
 * selection took, section 2h; -1 = none yet),
 * "forest_rounds_last" and "forest_edges_last" (the rounds the last selhip_ctx_spanning_forest call took and the edges F of its
 * forest, section 2j; -1 = none yet),
 * "linkage_rounds_last", "linkage_merges_last", "linkage_rowscans_last" and "linkage_rescans_last" (the rounds the last
 * selhip_ctx_linkage call took, its merges F, the rows it scanned and its rescan rounds, section 2k; -1 = none yet) */
int selhip_ctx_get_param(const selhip_ctx* ctx, const char* name, int* value);
/* Stage 2 grouping (default on): the pairs that reach the HLL-14 stage are bucketed by query row (counting sort) so
 * that waves running side by side on one XCD share their query row in L2.  0 = off (same kernel, list as produced). */
int selhip_ctx_set_stage2_grouping(selhip_ctx* ctx, int enable);
/* SELHIP_FP_FMA (default) or SELHIP_FP_STRICT */
int selhip_ctx_set_fp_mode(selhip_ctx* ctx, int fp_mode);

/* Host -> device upload of sketches already in ascending-cardinality order
 * (the flatten step of selection_cuda.cpp:131-143 + the H2D copies :167-169).
 *   h_hll [n][1<<p_hll] u8, h_aux [n][m] u64, h_cards [n] f64 (may be NULL: computed on the device
 *   from the registers with the Ertl-MLE estimator, == hll_t::report()).
 * p_hll is 4 .. 20.  What runs at p_hll != 14 (tests/test_hll_precision_host.py, tests/test_hll_precision_gpu.py: bit for bit
 * against the oracle at every p):
 *   entry                                              | at p_hll != 14
 *   ---------------------------------------------------+--------------------------------------------------------------------------
 *   upload / attach, selhip_hll_cards                  | no bit planes ("hll_khi" 0); cards from the byte rows
 *   selhip_ctx_run*, selhip_ctx_run_pairs*, top-k,     | stage 2 on byte rows through hll_union_hist_kernel: no bit-plane stage, no
 *   selhip_ooc_select, selhip_multi_select,            | grouping, no one-launch small pass ("small_pass_used" 0); same records and
 *   launch_kernel_*                                    | statistics as the oracle at that p
 *   selhip_hll_union_hist, selhip_ertl_estimate        | any p in 4 .. 20
 *   SELHIP_CRIT_NONE, HLL matrices, query passes       | refused: SELHIP_E_BADARG, they need p_hll = 14
 *
 * A context may be given one set after another, of any shape (tests/test_context_reuse_gpu.py).  A successful upload / attach
 *   RESETS  the results and statistics of the last pass (selhip_ctx_stats / _result_count / _fetch answer SELHIP_E_STATE until the
 *           next pass), the candidate begin (0), the queries with their auxiliary sketches (query passes: SELHIP_E_STATE until new
 *           queries are loaded), the database's auxiliary HLL sketches, uploaded, attached or folded (criteria that need them:
 *           SELHIP_E_STATE), the cached band signatures ("sig_cache"), the query side's database signatures and its index;
 *   KEEPS   criterion, measure, estimator, min_matches / min_containment, both top-k settings, the row rounds, the row
 *           interleave, the pipeline, stage-2 grouping, the fp mode, the stream and every selhip_ctx_set_param value.
 * Failure: every check that can refuse the call on its ARGUMENTS (shape, null or misaligned pointers, host cards that are not
 * finite, negative or not ascending) runs before the context is touched: after such a SELHIP_E_BADARG the context is exactly what
 * it was -- a used one still holds its database, queries, auxiliary sketches and results and its next pass gives the old set's
 * answer, a fresh one is still fresh.  A failure that shows only later (a HIP error while the rows are copied or the bit planes,
 * sparse lists or cards are built) leaves a context that holds NO database, after upload and attach alike: n = 0, the queries
 * dropped, a pass selects nothing until the next successful upload / attach. */
int selhip_ctx_upload(selhip_ctx* ctx, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards,
                      int64_t n_genomes, int m, int p_hll);
/* Same, for sketches that already live in device memory (caller keeps ownership and must keep them
 * alive while the context uses them).  d_cards may be NULL (computed). */
int selhip_ctx_attach(selhip_ctx* ctx, const uint8_t* d_hll, const uint64_t* d_aux, const double* d_cards,
                      int64_t n_genomes, int m, int p_hll);

/* Auxiliary HLL sketches (the .hll_<p> files, rank order, [n][1 << p_aux] u8) for the hll_a / hll_an criteria;
 * call after upload/attach of the primary sketches.  attach: device pointer owned by the caller. */
int selhip_ctx_upload_aux_hll(selhip_ctx* ctx, const uint8_t* h_aux_hll, int p_aux);
int selhip_ctx_attach_aux_hll(selhip_ctx* ctx, const uint8_t* d_aux_hll, int p_aux);
/* The same sketches without the .hll_<p> files: the context FOLDS them on the device from the main sketches it holds, uploaded or
 * attached, into a buffer it owns (hll_fold_kernel, see selhip_hll_fold in section 3: bit for bit the registers build_sketch writes
 * for p_aux from the same FASTA).  It leaves the context exactly as selhip_ctx_upload_aux_hll with that array would.  p_aux in
 * 4 .. min(p_hll, 15): SELHIP_E_BADARG with a message outside; SELHIP_E_STATE before upload / attach of the main sketches and while
 * a pass is pending.  Runs on the context's stream and returns when the sketches are there.  Like an upload it is replaced by the
 * next upload / attach / fold of auxiliary sketches.  It is a SNAPSHOT of the main sketches at the call and is NOT refreshed: a later
 * upload / attach of main sketches drops it like any auxiliary array (fold again), and rewriting an attached main buffer in place
 * leaves it stale, just as the bit planes and cards taken at selhip_ctx_attach are. */
int selhip_ctx_fold_aux_hll(selhip_ctx* ctx, int p_aux);
/* criterion used by the following selhip_ctx_run* calls (default SELHIP_CRIT_SMH_A); n_rows/n_bands are
 * ignored by HLL_A / HLL_AN / NONE (NONE ignores algo too and needs no auxiliary HLL sketches) */
int selhip_ctx_set_criterion(selhip_ctx* ctx, int criterion);
/* SELHIP_CRIT_SMH_C: a pair of the pass's pair space survives stage 1 iff c(i,k) = #{ j < m : aux_i[j] == aux_k[j] } >= c_min, compared
 * on the full 64 bits (two empty SuperMinHash rows count m); survivors go to the J test of every other criterion and records carry
 * the same J bits.  c_min < 1 is refused here (SELHIP_E_BADARG); a run under the criterion answers SELHIP_E_BADARG, naming it, when
 * c_min was never set, when c_min > m and when the context holds no SuperMinHash rows.  The value survives uploads / attaches.
 * stats[1] = stats[3] = the pairs of the pair space with c >= c_min.  All-pairs passes (row ranges, row interleave, candidate begin,
 * pipeline, all-pairs top-k), query passes and pair-list passes take the criterion; selhip_multi_select and selhip_ooc_select, whose
 * signatures carry no c_min, refuse it.  get_param "smhc_path_used": the stage-1 kernel of the last such pass, 1 = the fast path
 * (m = 128, 256, 512, 1024), 0 = the generic one, -1 = none yet.  The stage is timed as "stage1". */
int selhip_ctx_set_min_matches(selhip_ctx* ctx, int c_min);
/* SELHIP_CRIT_SMH_C with a PER-PAIR count threshold, for a minimum containment gamma.  With c / m the
 * SuperMinHash estimate of J, I = J (a + b) / (1 + J) and the containment estimate of the smaller genome is
 * C^ = I / a = c (a + b) / ((m + c) a), so C^ >= gamma iff c >= gamma m a / (a + b - gamma a).  The rule (csrc/pair_value.hpp, every
 * operation one IEEE-754 double operation, no contraction):
 *   smhc_threshold(m, gamma, e_lo, e_hi) -> int in [0, m + 1]        e_lo = min, e_hi = max of the pair's truncated cardinalities
 *       a = (double)e_lo, b = (double)e_hi
 *       if (a == 0) return m + 1                  (stage 2 never selects d = 0 under max containment; two empty rows do not survive)
 *       num = (gamma * (double)m) * a
 *       den = (a + b) - gamma * a
 *       if (!(den > 0)) return m + 1              (gamma >= 1 + b / a: no count reaches it)
 *       q = num / den
 *       return q <= 0 ? 0 : q > m ? m + 1 : (int)ceil(q)
 * A pair of the pass's pair space survives stage 1 iff c(i,k) >= max(c_min if set else 0, smhc_threshold(m, gamma, min(e_i, e_k),
 * max(e_i, e_k))): c_min (selhip_ctx_set_min_matches) stays as a floor -- for e_hi >> e_lo the threshold falls to a handful of buckets.
 * Sticky like set_min_matches and survives uploads; NaN clears it (the fixed rule again); +-inf is SELHIP_E_BADARG; SELHIP_E_STATE
 * while a pass is pending.  It takes effect under SELHIP_CRIT_SMH_C alone, where a run now needs c_min or gamma; c_min > m is still
 * refused.  A bucket prefilter, so taken under both measures and both modes (C^ >= gamma is also necessary for J >= gamma), by every
 * pass that takes the criterion.  stats[1] = stats[3] = the survivors of the exact rule.  get_param "smhc_rule_used": the rule of the
 * last such pass, 0 = fixed, 1 = containment, -1 = none yet. */
int selhip_ctx_set_min_containment(selhip_ctx* ctx, double gamma);
/* the rule above on the host (no device is touched): what the kernels compute for one pair */
int selhip_smhc_threshold(int m, double gamma, uint64_t e_lo, uint64_t e_hi);
/* The MEASURE that stage 2 of the following passes tests against tau_f and records (sticky like the criterion; survives uploads):
 *   SELHIP_MEASURE_JACCARD (default)    J = I / U with I = (double)e_i + (double)e_k - U      (selection.cpp:287; nothing changes)
 *   SELHIP_MEASURE_MAX_CONTAINMENT      V = I / d, d = min(e_i, e_k): the share of the SMALLER genome found in the larger one -- the
 *                                       measure for pairs of unequal size (a plasmid, phage or fragment inside a genome, a draft inside
 *                                       its complete assembly), whose J can never exceed e_small / e_large.
 * I is J's numerator as the kernels spell it (left to right, f64, no fused operation), so J and I / U share their bits; no clamp and
 * no abs, as for J: estimator noise may give V < 0 or V > 1.  A pair that reaches stage 2 is selected iff d != 0 && V >= (double)tau_f
 * and its record is {i, k, V}: the `jaccard` field of selhip_pair_t carries the measure.  The pair spaces stay as they are and so do
 * stats[0..3]; a pair with d == 0 counts as evaluated and as a survivor and is never selected.  The measure is symmetric, so the
 * invariant of the query passes holds (records = the cross pairs of the all-pairs result over Q u D) and the order of an entry's
 * ranks in a pair list does not matter.  Taken by selhip_ctx_run / _run_async (row ranges, row interleave, candidate begin, pipeline),
 * selhip_ctx_run_queries, selhip_ctx_run_pairs / _async and the two top-ks behind them (which rank by the record's value, ties as
 * before), under SELHIP_CRIT_NONE, _SMH_C and _SMH_A with every algorithm.  smh_a and smh_c are prefilters on bucket equality, tuned
 * for J: in front of the containment test they cost recall on pairs of unequal size -- the caller's choice.
 * Refused with SELHIP_E_BADARG and a message naming the measure, before anything is enqueued (the context stays fully usable):
 *   SELHIP_MODE_CB_SMH -- the CB bound e_small / e_large >= tau is a bound on J and would cut exactly the pairs this measure exists
 *   for: pass SELHIP_MODE_SMH --, and SELHIP_CRIT_HLL_A, _HLL_AN, _HLL_A_SMH_A, whose bounds are derived for J.
 * Any other measure code: SELHIP_E_BADARG.  SELHIP_E_STATE while a pass is pending.  The one-launch pass of a small set has the J
 * test only: under max containment the regular pass runs (get_param "small_pass_used" reads 0).  The drop-in launchers,
 * selhip_multi_select and selhip_ooc_select carry no measure: J.  A context that never calls this launches what it always did. */
int selhip_ctx_set_measure(selhip_ctx* ctx, int measure);
/* The ESTIMATOR behind the value that the following passes test against tau_f and record (sticky like the
 * measure; survives uploads):
 *   SELHIP_ESTIMATOR_HLL (default)   the HLL estimate of stage 2, as described above: nothing changes, the same launches as before
 *   SELHIP_ESTIMATOR_SMH             the SuperMinHash estimate, a function of the count c(i,k) of equal buckets that a pass of
 *                                    SELHIP_CRIT_SMH_C already computes for every pair it admits, of m and of the pair's truncated
 *                                    cardinalities e_i, e_k alone (csrc/pair_value.hpp, every operation one IEEE-754 double operation,
 *                                    no contraction):
 *   smh_value(measure, m, c, e1, e2) -> double
 *       SELHIP_MEASURE_JACCARD          V = (double)c / (double)m
 *       SELHIP_MEASURE_MAX_CONTAINMENT  a = (double)min(e1, e2), b = (double)max(e1, e2)
 *                                       V = ((double)c * (a + b)) / (((double)m + (double)c) * a)     -- the estimate C^ behind
 *                                       selhip_smhc_threshold; min(e1, e2) == 0 gives NaN explicitly (never selected); no clamp: V may
 *                                       exceed 1, as every containment value of this library may
 *       any other measure               NaN
 * Under SELHIP_ESTIMATOR_SMH a pass selects a pair iff (1) it lies in the pass's pair space E -- unchanged: rank order, e_k != 0, the
 * CB window under SELHIP_MODE_CB_SMH, the own E of query and pair-list passes --, (2) c >= the pass's count threshold -- unchanged:
 * the fixed c_min, or the per-pair rule of selhip_ctx_set_min_containment with c_min as its floor -- and (3) V >= (double)tau_f.  Its
 * record is {i, k, V} in the index space of the pass kind.  The count floor of such a pass is 1 whatever the rule gives (c_min >= 1;
 * a gamma <= 0 without c_min asks for 0): a pair with c < 1 never has a record.  Stage 1 emits the records itself: the pass is its
 * bounds / windows kernel, the count kernel and the counter copy -- nothing is grouped, no union histogram and no estimate is launched,
 * no HLL register or bit plane is read.  stats[0] = the evaluated pairs, stats[1] = stats[3] = the pairs with c >= their threshold,
 * stats[2] = the records.  Row ranges, row interleave, candidate begin, pipeline lanes, the growth of a result list that overflowed,
 * both top-k cuts (which rank by V; c / m is discrete, so ties -- broken by ascending partner rank as ever -- are common), fetch,
 * fetch_ranked, copy_results* and get_param "smhc_path_used" / "smhc_rule_used" work as for the criterion under the HLL estimator.
 * Refused with SELHIP_E_BADARG and a message naming the estimator, by every run entry before anything is enqueued: SELHIP_ESTIMATOR_SMH
 * with a criterion other than SELHIP_CRIT_SMH_C; besides, everything the criterion and the measure refuse on their own (max containment
 * still takes no SELHIP_MODE_CB_SMH).  Any other estimator code: SELHIP_E_BADARG with a message, the setting is left alone.
 * SELHIP_E_STATE while a pass is pending.  selhip_multi_select and selhip_ooc_select refuse smh_c and so carry no estimator; a context
 * still uploads its HLL rows. */
#define SELHIP_ESTIMATOR_HLL 0
#define SELHIP_ESTIMATOR_SMH 1
int selhip_ctx_set_estimator(selhip_ctx* ctx, int estimator);
/* smh_value above on the host (no device is touched): what the kernels compute for one pair */
double selhip_smh_value(int measure, int m, int c, uint64_t e1, uint64_t e2);

/* report() of every genome (Ertl-MLE, hll.h:834-837,862) computed on the device: d_cards_out[n]. */
int selhip_hll_cards(selhip_ctx* ctx, const uint8_t* d_hll, int64_t n_genomes, int p, double* d_cards_out);
/* copies the context's cardinalities to the host */
int selhip_ctx_get_cards(selhip_ctx* ctx, double* h_cards_out);

/* One pass of the hot path over query rows [row_begin, row_end) (0, n_genomes = everything;
 * a sub-range is one rank's shard of the pair space: rows are independent).
 * tau_f is the FLOAT threshold of the reference (`float threshold`, selection.cpp:81,103).
 * Results stay on the device until fetched.  Synchronous w.r.t. the context's stream on return. */
int selhip_ctx_run(selhip_ctx* ctx, int mode, int algo, float tau_f, int n_rows, int n_bands,
                   int64_t row_begin, int64_t row_end);
/* Asynchronous variant: enqueues the pass and returns; selhip_ctx_finish() waits and validates. */
int selhip_ctx_run_async(selhip_ctx* ctx, int mode, int algo, float tau_f, int n_rows, int n_bands,
                         int64_t row_begin, int64_t row_end);
int selhip_ctx_finish(selhip_ctx* ctx);

/* statistics of the last finished run:
 *   stats[0] pairs evaluated by the smh_a predicate (after e_k==0 / CB pruning)
 *   stats[1] pairs that passed the auxiliary criterion/criteria (smh_a: pairs with a fully equal band)
 *   stats[2] selected pairs (J >= tau)
 *   stats[3] candidates produced by the signature join (ALGO_SIG; = stats[1] for ALGO_STREAM)
 * SELHIP_CRIT_NONE: the empty criterion passes everything, stats[1] = stats[3] = stats[0]. */
int selhip_ctx_stats(const selhip_ctx* ctx, int64_t stats[4]);
int64_t selhip_ctx_result_count(const selhip_ctx* ctx);
/* copies min(count, cap) records to the host, sorted by (i,k) = the reference's print order */
int selhip_ctx_fetch(selhip_ctx* ctx, selhip_pair_t* h_out, int64_t cap);
/* device-side view of the unsorted result list (for RCCL gathers without a host round trip) */
int selhip_ctx_result_device(selhip_ctx* ctx, const selhip_pair_t** d_results, int64_t* count);
/* device-to-device copy of min(count, cap) unsorted records into caller memory (e.g. a torch tensor that
 * is then handed to an RCCL collective); asynchronous on the context's stream. */
int selhip_ctx_copy_results(selhip_ctx* ctx, selhip_pair_t* d_dst, int64_t cap);
/* same, framed for a fixed-size collective: d_dst[0] = 16-byte header {u64 count, u64 0}, records from d_dst + 16;
 * d_dst must hold cap_records + 1 records.  Returns SELHIP_E_OVERFLOW (after copying cap_records) if count > cap. */
int selhip_ctx_copy_results_framed(selhip_ctx* ctx, void* d_dst, int64_t cap_records);
/* The same frame, enqueued BEHIND a pass that is still running (between selhip_ctx_run_async and selhip_ctx_finish), so
 * that the caller can also enqueue its collective before it waits: the count is not known on the host yet, so one small
 * kernel reads the device-side counter, writes the header and copies min(count, cap_records) records (d_dst 16-byte
 * aligned).  After selhip_ctx_finish the caller checks selhip_ctx_result_count() <= cap_records and
 * selhip_ctx_last_attempts() == 1 (an overflowing internal list makes finish repeat the pass, which would leave the
 * frame stale) and otherwise frames again. */
int selhip_ctx_copy_results_framed_async(selhip_ctx* ctx, void* d_dst, int64_t cap_records);
/* number of times the last finished run had to enqueue its pass (1 = no internal list overflowed) */
int selhip_ctx_last_attempts(const selhip_ctx* ctx);

/* Top-k of the all-pairs passes: every genome keeps only its k best partners, cut and ordered on the device behind the pass.
 *   S = the result of an all-pairs pass (selhip_ctx_run, or selhip_ctx_run_async + selhip_ctx_finish) as described above: any criterion,
 *   mode, algorithm, row range, row interleave, candidate begin or chunk count, and the one-launch small pass; records {i, k, J}, i < k.
 *   The DIRECTED LIST D(S) holds two records for every record (i, k, J) of S: {owner i, partner k, J} and {owner k, partner i, J} -- a
 *   pair belongs to both genomes' lists.  Within one owner, record a RANKS BEFORE record b iff key(a.J) > key(b.J), or the keys are
 *   equal and a.partner < b.partner, with the sort key of section 2b (selhip_ctx_set_query_topk); partners are unique within an owner,
 *   so the order is strict and total.  nbr(S, k) keeps, for every genome g in 0 .. n - 1, the first min(L_g, k) records of that ranking
 *   (L_g = the records of S with i = g or k = g).  Its RANKED ORDER is owner ascending, then ranking order; its records are
 *   selhip_pair_t {i = owner, k = partner, jaccard}, J bits unchanged.  The reduced count, the sum of min(L_g, k) over all genomes, can be
 *   LARGER than |S| (up to 2 |S|): a selected pair appears twice, once or not at all.
 * As for queries this is the k best among the pairs that pass the criterion and tau_f; for every genome's exact nearest neighbours use
 * SELHIP_CRIT_NONE with SELHIP_MODE_SMH and a tau_f below every J, e.g. -1 (selhip_ctx_run_async puts no bound on tau_f).
 * selhip_ctx_set_allpairs_topk: k = 0 switches the cut off (the default: an all-pairs pass issues exactly the launches and returns
 * exactly the bytes it did without this call), 1 .. SELHIP_TOPK_MAX switches it on; anything else SELHIP_E_BADARG; SELHIP_E_STATE while
 * a pass is pending.  The setting survives uploads / attaches and is read by the all-pairs passes of this context only: query passes
 * ignore it as all-pairs passes ignore selhip_ctx_set_query_topk, and selhip_multi_select, selhip_ooc_select and the drop-in launchers
 * use contexts of their own.
 * With k > 0 selhip_ctx_finish, once the pass is accepted (every list fitted), replaces the context's result list with nbr(S, k) in
 * ranked order, on the context's stream: selhip_ctx_result_count returns the reduced count, selhip_ctx_fetch the reduced list sorted by
 * (i, k), selhip_ctx_fetch_ranked / selhip_ctx_result_device / selhip_ctx_copy_results give it as it lies; selhip_ctx_stats and
 * selhip_ctx_last_attempts are unchanged (stats[2] stays |S|).  selhip_ctx_copy_results_framed / _framed_async return SELHIP_E_STATE
 * while the setting is on: their header is the device-side |S| counter.  With the setting off selhip_ctx_fetch_ranked after an all-pairs
 * pass returns SELHIP_E_STATE as before.
 * A pass that selected nothing launches nothing more.  At most 2^31 - 1 directed records, 2 |S|, per pass (SELHIP_E_BADARG beyond).  The
 * cut's scratch is 12 bytes per directed record, and the result buffer grows when the reduced count exceeds it; if either cannot be
 * allocated the call returns SELHIP_E_HIP and the pass counts as not run.  The cut is timed as "topk" (not part of "total").
 * SELHIP_TOPK_MAX and selhip_ctx_fetch_ranked are declared in section 2b. */
int selhip_ctx_set_allpairs_topk(selhip_ctx* ctx, int k);

/* The all-pairs top-k in ROW ROUNDS: nbr(S, k) without ever holding S.  For the all-pairs passes with selhip_ctx_set_allpairs_topk(k > 0),
 * SELHIP_CRIT_SMH_C and SELHIP_ESTIMATOR_SMH (the passes whose stage 1 emits the records).  The pass's row range is cut into rounds
 * of `rows` rows; each round runs as the sub-range pass a caller could run, its records are merged into a carried directed list C of at
 * most k records per genome, and
 *     thr[g] = -inf while C holds fewer than k records of owner g, else the value of g's k-th record in C
 * is raised from C.  A pair (i, k') of a later round that passes everything it passes in the one-shot pass (pair space, count threshold,
 * V >= tau_f) is ADMITTED -- appended and merged -- iff V >= thr[i] || V >= thr[k'], with the thresholds as they stood when its round
 * began; every other pair is dropped where it is counted.  The test is not strict: a tie with the k-th value can displace it by partner
 * rank.  The result is nbr(S, k) of the one-shot pass, record for record and bit for bit, in ranked order (a pair rejected for owner g
 * has k records of g ranking before it, and thresholds only rise); memory is n k records plus one round's admitted records instead
 * of |S|, and the limit of 2^31 - 1 directed records applies to |C| + 2 (admitted records of one round) instead of 2 |S|.
 * rows = 0: off (the default: every pass issues exactly the launches and returns exactly the bytes it does without this call);
 * rows > 0: that many rows per round; SELHIP_TOPK_ROUNDS_AUTO: the largest R with R n <= 2^27 records, one row at least.  Under a row
 * interleave of more than one part a round is whole periods of the deal (2 block_rows n_parts rows): rows is rounded up to that.
 * Anything else SELHIP_E_BADARG; SELHIP_E_STATE while a pass is pending.  The setting survives uploads / attaches.  Only all-pairs passes
 * read it: query passes and pair-list passes ignore it, and an all-pairs pass with rounds on but without the all-pairs top-k, criterion
 * smh_c or the estimator smh is refused with SELHIP_E_BADARG before anything is launched.
 * selhip_ctx_run_async enqueues the first round, selhip_ctx_finish drives the rest; a round whose result list overflows grows the list
 * and repeats alone.  Row interleave, candidate begin and selhip_ctx_set_pipeline apply inside each round.  Afterwards the result
 * accessors behave as behind any cut pass; selhip_ctx_stats returns what the one-shot pass returns (stats[2] = |S|, the pairs with
 * V >= tau_f, not the admitted count); selhip_ctx_last_attempts is the largest attempt count of any round.  selhip_ctx_get_param:
 * "topk_rounds" (the setting), "topk_rounds_used" (rounds of the last all-pairs pass, 0 = it ran in one), "topk_admitted_lo" /
 * "topk_admitted_hi" (low / high 31 bits of the records admitted over all rounds).  Merge and thresholds are timed as "topk". */
#define SELHIP_TOPK_ROUNDS_AUTO (-1)
int selhip_ctx_set_topk_rounds(selhip_ctx* ctx, int64_t rows);

/* device time (ms, HIP events on the stream each kernel is launched on) of the named kernel PER PASS, averaged over
 * the passes since the last reset (a pipelined pass launches a kernel once per row chunk: the figure is their sum);
 * names: "prep", "sigbuild", "join", "verify", "stage1", "aux", "group", "hist", "select", "dense" (the fused kernel of
 * SELHIP_CRIT_NONE), "topk" (the cut of a query pass with selhip_ctx_set_query_topk, section 2b: its four launches; not part of "total"), "total"; "join_span" = first start to
 * last end of the pass's join launches (chunk lanes run them side by side).  <0 if never launched.
 * "topk" is also the cut of an all-pairs pass with selhip_ctx_set_allpairs_topk (above), again outside "total".
 * "matrix" is the kernel of a dense matrix (section 2f), averaged over the MATRIX CALLS since the last reset: they are counted apart
 * from the passes, so a matrix call changes no other name's per-pass figure.  "matrix_smh" is the kernel of a matrix call with a
 * SuperMinHash measure, averaged over THOSE calls: "matrix" stays the HLL kernel's figure and count.
 * "cluster" is the launches of selhip_ctx_cluster (section 2g), averaged over the CLUSTER CALLS since the last reset, counted apart likewise.
 * "greedy" is the launches of selhip_ctx_cluster_greedy (section 2h), averaged over the GREEDY CALLS since the last reset, counted apart likewise.
 * "merge" is the launches of selhip_ctx_merge_groups (section 2i), averaged over the MERGE CALLS since the last reset, counted apart likewise.
 * "forest" is the launches of selhip_ctx_spanning_forest (section 2j), averaged over the FOREST CALLS since the last reset, counted apart likewise.
 * "linkage" is the launches of selhip_ctx_linkage (section 2k: the matrix kernel that fills its scratch, then the rounds), averaged over the
 * LINKAGE CALLS since the last reset, counted apart likewise; "matrix" and "matrix_smh" do not see that call.
 * selhip_ctx_kernel_launches: launches of that kernel per pass. */
double selhip_ctx_kernel_ms(const selhip_ctx* ctx, const char* name);
double selhip_ctx_kernel_launches(const selhip_ctx* ctx, const char* name);
/* enable: 0 = off, 1 = every kernel scope, 2 = only ONE kernel: the stage-1 kernel ("join" for the signature algorithms,
 * "stage1" otherwise; "dense" for SELHIP_CRIT_NONE) or, after selhip_ctx_set_param(ctx, "timed_kernel", 1), stage 2a ("hist") -- an event pair costs ~10 us of
 * stream time, so level 2 is what a throughput measurement leaves on, on whichever kernel is the longest of the step.
 * Every call resets the accumulated figures. */
int    selhip_ctx_timing(selhip_ctx* ctx, int enable);

/* ---------------------------------------------------------------------------------------------------
 * 2b. Query passes: a query set Q against the context's sketches (the database D).  Both sets are in ascending-cardinality
 *     order, with the same m and p = 14.  A pass selects the pairs (q, d) -- q a query rank, d a database rank -- with
 *     e_hi != 0, [CB mode] (double)e_lo / (double)e_hi >= (double)tau_f, the criterion set with selhip_ctx_set_criterion and
 *     J >= tau_f (e_lo / e_hi = the smaller / larger of the two truncated cardinalities; same estimator and FP flavour as
 *     selhip_ctx_run).  The auxiliary criteria hll_a / hll_an take card_A <= card_B (gamma = e_A / e_B, e_B on its own): a
 *     query pair passes (e_lo, e_hi) in that order, whichever set each member comes from; every other term is symmetric.  So
 *     the result is exactly the cross pairs (one member in Q, one in D) of selhip_ctx_run over Q u D, J bit for bit, for
 *     every criterion: SELHIP_CRIT_SMH_A, _HLL_A, _HLL_AN, the two-stage _HLL_A_SMH_A and _NONE (every (q, d) with d inside q's
 *     CB window -- SELHIP_MODE_SMH: every d -- and e_hi != 0 goes to the J test; algo, n_rows and n_bands are ignored).
 *     Records {i = query rank, k = database rank, jaccard} are read with selhip_ctx_result_count / _fetch (sorted by (i,k)),
 *     (both of the k best per query when selhip_ctx_set_query_topk is on, see below),
 *     selhip_ctx_stats (evaluated = cross pairs inside the CB windows with e_hi != 0; survivors = the cross pairs that pass the
 *     criterion before the J test -- smh_a, hll_a / hll_an, or both for the two-stage criterion, as selhip_ctx_run reports them)
 *     and selhip_ctx_last_attempts.
 *     Criteria other than smh_a and none need the auxiliary HLL sketches of both sets (selhip_ctx_upload_aux_hll for D,
 *     selhip_ctx_upload_queries_aux_hll for Q; SELHIP_E_STATE without them) with the same p_aux (SELHIP_E_BADARG otherwise).
 *     Where the smh_a stage runs (smh_a, two-stage) n_rows * n_bands must be m and algo is: SELHIP_ALGO_SIG (power-of-two
 *     rows, 8..128 bands: band signatures of a query tile in LDS against the database's, which are kept for the band shape
 *     used last -- a pass with the same shape against the same database does not build them again, one with another shape
 *     replaces them; get_param "query_db_sig_builds" counts the builds since the database was loaded), SELHIP_ALGO_STREAM
 *     (any band shape, m <= 4096: full bucket compare), SELHIP_ALGO_AUTO (SIG where it applies, else STREAM), or
 *     SELHIP_ALGO_INDEX (the band shapes of SIG; any other: SELHIP_E_BADARG, no fallback): the database's signatures sorted per
 *     band with their ranks plus a bucket directory per band, 9 to 10 bytes per (genome, band) (get_param "query_db_index_kib":
 *     its resident KiB), searched once per (query, band) instead of compared with every query --
 *     same records (J bit for bit), statistics and selhip_ctx_last_attempts as SIG.  The index is built by the first INDEX pass
 *     for (database, n_rows, n_bands) and kept: new queries, another tau with the same shape, another mode, and SIG / STREAM /
 *     all-pairs passes in between neither rebuild nor disturb it; another band shape replaces it; uploading / attaching the
 *     database drops it (get_param "query_db_index_builds" counts the builds since the database was loaded).  It is sorted from
 *     the database signatures SIG keeps, so switching between SIG and INDEX with one shape builds those once.  The probe is
 *     timed as "join", the index build as "sigbuild" (with the database signature build when that runs).
 *     SELHIP_ALGO_HASHJOIN is refused.  hll_a / hll_an alone ignore n_rows, n_bands and algo, as selhip_ctx_run does: each
 *     query's CB window of D is tested directly, without a pair list.  The auxiliary stage is timed as "aux".
 *     Uploading / attaching the database drops the queries; uploading / attaching the queries drops their auxiliary sketches.
 *     Query and all-pairs passes do not affect each other's results.
 *     After a query pass selhip_ctx_copy_results_framed / _framed_async return SELHIP_E_STATE (use selhip_ctx_copy_results).
 * --------------------------------------------------------------------------------------------------- */
/* h_cards / d_cards may be NULL (computed on the device, as selhip_ctx_upload does); n_q == 0 is legal (0 results).  Cards that are
 * not ascending: SELHIP_E_BADARG (host cards here, device cards at the run).  attach: device pointers owned by the caller. */
int selhip_ctx_upload_queries(selhip_ctx* ctx, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards, int64_t n_q);
int selhip_ctx_attach_queries(selhip_ctx* ctx, const uint8_t* d_hll, const uint64_t* d_aux, const double* d_cards, int64_t n_q);
/* Auxiliary HLL sketches of the query set, [n_q][1 << p_aux] u8 in query rank order, p_aux in 4..15 (as selhip_ctx_upload_aux_hll); after
 * selhip_ctx_upload_queries / _attach_queries (SELHIP_E_STATE before).  attach: 16-byte aligned device pointer owned by the caller.
 * The pointer may be NULL when n_q == 0. */
int selhip_ctx_upload_queries_aux_hll(selhip_ctx* ctx, const uint8_t* h_aux_hll, int p_aux);
int selhip_ctx_attach_queries_aux_hll(selhip_ctx* ctx, const uint8_t* d_aux_hll, int p_aux);
/* selhip_ctx_fold_aux_hll for the query set: its auxiliary sketches folded on the device from the queries' main sketches into a buffer
 * the context owns, under the rules of selhip_ctx_upload_queries_aux_hll (SELHIP_E_STATE before the queries are loaded or while a pass
 * is pending, SELHIP_E_BADARG with a message for p_aux outside 4..14; dropped by the next upload / attach of queries or database). */
int selhip_ctx_fold_queries_aux_hll(selhip_ctx* ctx, int p_aux);
/* One query pass, synchronous like selhip_ctx_run; SELHIP_E_STATE before any queries are loaded. */
int selhip_ctx_run_queries(selhip_ctx* ctx, int mode, int algo, float tau_f, int n_rows, int n_bands);

/* Top-k of the query passes: every query keeps only its k best records, cut and ordered on the device behind the pass.
 *   S = the result of a query pass as described above.  The sort key of a double J with bit pattern b is the u64
 *   b ^ 0x8000000000000000 if b's sign bit is clear and ~b if it is set: its unsigned order is the IEEE total order (NaN never passes
 *   J >= tau_f, and -0.0 cannot arise from (e_lo + e_hi - U) / U).  Within one query, record a RANKS BEFORE record b iff
 *   key(a.J) > key(b.J), or the keys are equal and a.k < b.k -- database ranks are unique within a query, so this is a strict total
 *   order and the answer is unique.  topk(S, k) keeps, for every query i, the first min(L_i, k) records of that ranking (L_i = the
 *   records of query i in S).  The RANKED ORDER of a list is i ascending, then ranking order.
 * The answer is "the k best among the pairs that pass the criterion and tau_f", not an unconditional k-nearest-neighbour search: a
 * criterion (smh_a, hll_a, ...) or a threshold that drops a pair drops it here too.  For exact nearest neighbours use SELHIP_CRIT_NONE
 * with SELHIP_MODE_SMH and a tau_f below every J (negative thresholds are legal in query passes; every J is above -1).
 * selhip_ctx_set_query_topk: k = 0 switches the cut off (the default: a query pass is exactly what it was without this call),
 * 1 .. SELHIP_TOPK_MAX switches it on; anything else SELHIP_E_BADARG; SELHIP_E_STATE while a pass is pending.  The setting survives
 * uploads / attaches and is read by selhip_ctx_run_queries only -- all-pairs passes, selhip_multi_select and selhip_ooc_select never cut.
 * With k > 0 selhip_ctx_run_queries, once the pass is accepted (every list fitted), replaces the context's result list with
 * topk(S, k) in ranked order, on the context's stream: selhip_ctx_result_count returns the reduced count, selhip_ctx_fetch the
 * reduced list in (i, k) order, selhip_ctx_result_device / selhip_ctx_copy_results expose it in ranked order; selhip_ctx_stats is
 * unchanged (stats[2] = |S|: the difference to selhip_ctx_result_count is what was cut), and so is selhip_ctx_last_attempts.
 * A pass that selected nothing launches nothing more.  If the cut's scratch (12 bytes per record of S) cannot be allocated the
 * call returns SELHIP_E_HIP and the pass counts as not run.  At most 2^31 - 1 records per pass (SELHIP_E_BADARG beyond).
 * get_param "query_topk" = the current k, "query_topk_lds_cap" = the longest segment (records of one query) the select kernel stages
 * in LDS; longer segments are streamed from global memory by every pass of the selection.  The cut is timed as "topk". */
#define SELHIP_TOPK_MAX 1024
int selhip_ctx_set_query_topk(selhip_ctx* ctx, int k);
/* copies min(count, cap) records of the reduced list as it lies -- ranked order, no host sort; SELHIP_E_STATE unless the last
 * finished pass was a query pass with top-k on; SELHIP_E_OVERFLOW (after copying cap records) if count > cap.
 * An all-pairs pass with selhip_ctx_set_allpairs_topk on (section 2) leaves a ranked list too, read the same way. */
int selhip_ctx_fetch_ranked(selhip_ctx* ctx, selhip_pair_t* h_out, int64_t cap);

/* ---------------------------------------------------------------------------------------------------
 * 2c. Multi-GPU entry taking a device list: ONE process, one host thread + one context per
 *     device; the pair space is cut into equal-pair row ranges, every device gets a full replica of the (host)
 *     sketches, and the selected-pair lists are gathered -- over RCCL/xGMI (ncclAllGather of framed record buffers on
 *     communicators from ncclCommInitAll; librccl is dlopen'ed on first use) or through the host.
 *     Any criterion (SELHIP_CRIT_*): h_aux_hll / p_aux carry the auxiliary HLL sketches of hll_a, hll_an and the two-stage
 *     criterion of BASELINE configs[4] (NULL / 0 for smh_a and for SELHIP_CRIT_NONE).  Rows are dealt to the devices in interleaved blocks of 128
 *     (selhip_ctx_set_row_interleave).  h_out receives min(count, cap) records sorted by (i,k); stats_out (optional) as
 *     selhip_ctx_stats.
 * --------------------------------------------------------------------------------------------------- */
#define SELHIP_GATHER_HOST           0   /* each device's list is fetched and merged on the host              */
#define SELHIP_GATHER_RCCL           1   /* RCCL all_gather; an error if RCCL cannot be initialised           */
#define SELHIP_GATHER_RCCL_OR_HOST   2   /* RCCL if it initialises, host merge otherwise (note in last_error) */
int selhip_multi_select(const int* devices, int n_devices,
                        const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards,
                        const uint8_t* h_aux_hll, int p_aux, int criterion,
                        int64_t n_genomes, int m, int p_hll, int mode, int algo, int fp_mode, float tau_f, int n_rows, int n_bands,
                        int gather, selhip_pair_t* h_out, int64_t cap, int64_t* count_out, int64_t stats_out[4]);

/* ---------------------------------------------------------------------------------------------------
 * 2d. Out-of-core driver: the sketches stay in HOST memory (all n genomes, ascending
 *     cardinality, h_cards required) and only `block_genomes` of them per block are resident on the device at a time.
 *     The pair space is tiled into block pairs (I, J), I <= J: a diagonal block is an ordinary pass over I; an
 *     off-diagonal one uploads I followed by J and runs rows I x candidates J (selhip_ctx_set_candidate_begin), so every
 *     pair is evaluated exactly once and the result -- pairs, Jaccard values, statistics -- is identical to one in-core
 *     pass over the whole set.  n_streams = 2 runs two block pairs at a time (own buffers, own context, own host thread):
 *     the upload of one overlaps the pass of the other; device memory needed ~ n_streams * 2 * block_genomes sketches.
 *     h_aux_hll/p_aux are only needed for the criteria with an auxiliary-HLL stage (NULL/0 for SELHIP_CRIT_SMH_A and _NONE).
 *     h_out receives min(count, cap) records with GLOBAL ranks, sorted by (i,k); SELHIP_E_OVERFLOW (count still exact)
 *     if cap was too small.
 * --------------------------------------------------------------------------------------------------- */
int selhip_ooc_select(int device, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards,
                      const uint8_t* h_aux_hll, int p_aux, int criterion,
                      int64_t n, int m, int p_hll, int mode, int algo, int fp_mode, float tau_f, int n_rows, int n_bands,
                      int64_t block_genomes, int n_streams,
                      selhip_pair_t* h_out, int64_t cap, int64_t* count_out, int64_t stats_out[4]);

/* ---------------------------------------------------------------------------------------------------
 * 2e. Pair-list passes: the context's criterion over a CALLER'S list of pairs instead of the whole triangle -- re-scoring an
 *     earlier result under another criterion or threshold, candidates from another tool, J of given pairs (SELHIP_CRIT_NONE,
 *     SELHIP_MODE_SMH, tau_f = -1).
 *     Let E be the pair space an all-pairs pass over all rows evaluates -- (i, k), i < k, e_k != 0, and in SELHIP_MODE_CB_SMH the CB
 *     predicate -- and S that pass's result.  d_pairs holds n_pairs entries {x, y} in device memory (8-byte aligned), each naming
 *     the unordered pair of the ranks x and y; 0 <= n_pairs <= 2^31 - 1.  The result is one record {min, max, J} for every entry
 *     whose pair is in S, with the J of S bit for bit; an entry listed twice is evaluated and reported twice; selhip_ctx_fetch
 *     sorts by (i, k) as always.  An entry with x == y or a rank outside [0, n) makes the pass fail: selhip_ctx_finish returns
 *     SELHIP_E_BADARG, the message gives the number of such entries and the index of one, and the context holds no results
 *     (selhip_ctx_stats: SELHIP_E_STATE).
 *     Statistics count ENTRIES: stats[0] entries whose pair is in E, stats[1] entries passing the criterion (meaning per criterion as
 *     for an all-pairs pass), stats[2] records, stats[3] on the signature route the entries in E with an equal 32-bit band signature,
 *     = stats[1] otherwise (SELHIP_CRIT_NONE: stats[1] = stats[3] = stats[0]).
 *     d_pairs stays the caller's: alive and unchanged until selhip_ctx_finish returns (a pass that outgrows one of its lists is
 *     repeated and reads it again), visible to the context's stream at the call.  n_pairs == 0 is a finished pass without records.
 *     Arguments are checked as by selhip_ctx_run_async.  algo picks stage 1 of the criteria with an smh_a stage: SELHIP_ALGO_SIG the
 *     signature route (band signatures built like an all-pairs pass's, then one check per entry; SELHIP_E_BADARG for a band shape
 *     without signatures), SELHIP_ALGO_STREAM the direct route (the band comparison on the sketches, any band shape),
 *     SELHIP_ALGO_AUTO the signature route where the shape has one and the signatures are cached ("sig_cache") or n_pairs >= n / 2;
 *     SELHIP_ALGO_HASHJOIN and _INDEX are joins, not checks of a given pair: SELHIP_E_BADARG.  SELHIP_E_STATE with the all-pairs
 *     top-k on (selhip_ctx_set_allpairs_topk), a row interleave of more than one part, or a candidate begin above 0: shard a list
 *     by cutting the list.
 *     To everything that follows, a list pass is an all-pairs pass: fetch, result_device, copy_results*, last_attempts, kernel_ms
 *     (its stage-1 kernel is "stage1"); get_param "chunks" = 1, "small_pass_used" = 0, and "pairs_route_used" = 1 signature route,
 *     0 direct route, 2 criterion without an smh_a stage, -1 no list pass yet.
 * --------------------------------------------------------------------------------------------------- */
int selhip_ctx_run_pairs(selhip_ctx* ctx, const selhip_int2_t* d_pairs, int64_t n_pairs,
                         int mode, int algo, float tau_f, int n_rows, int n_bands);
/* Asynchronous variant: selhip_ctx_finish() waits, validates and reports invalid entries. */
int selhip_ctx_run_pairs_async(selhip_ctx* ctx, const selhip_int2_t* d_pairs, int64_t n_pairs,
                               int mode, int algo, float tau_f, int n_rows, int n_bands);

/* ---------------------------------------------------------------------------------------------------
 * 2f. Dense matrices: the similarity of EVERY pair as one array in the caller's device memory (what `mash triangle` / `dashing dist`
 *     print), no criterion, no threshold, no record list.  The cell of a row genome a and a column genome b:
 *       U = the Ertl estimate of the register-wise maximum of the two p = 14 sketches, in the context's FP flavour
 *           (the reference's hll_t::union_size; the arithmetic of the passes' stage 2);
 *       SELHIP_MEASURE_UNION stores U; SELHIP_MEASURE_JACCARD stores ((double)e_a + (double)e_b - U) / U (selection.cpp:287, e = the
 *       truncated cardinalities) for every pair without exception: two empty sketches give NaN, and the matrix holds that NaN.
 *     On the diagonal of a self matrix UNION stores U(i, i), computed like any cell; JACCARD stores exactly 1.0.  dtype SELHIP_F64
 *     carries the bits the passes' records carry, SELHIP_F32 is (float) of that value.  A self matrix is bit-symmetric.
 *     Three more measures come from the same U and the same numerator I = (double)e_a + (double)e_b - U (csrc/pair_value.hpp):
 *       SELHIP_MEASURE_INTERSECTION stores I, the inclusion-exclusion estimate of |A n B|; its diagonal is computed like any cell;
 *       SELHIP_MEASURE_CONTAINMENT stores I / e_a, the share of the ROW genome found in the column genome -- in a query matrix the
 *       query inside the database genome, the question of `mash screen`.  It is NOT symmetric; it is NaN when e_a == 0; on the
 *       diagonal of a self matrix it is exactly 1.0.  A self matrix still computes each pair once: the mirrored store at (b, a)
 *       writes I / e_b from the same U, bit-equal to that cell computed on its own (IEEE addition commutes);
 *       SELHIP_MEASURE_MAX_CONTAINMENT stores I / min(e_a, e_b), the value the passes record after selhip_ctx_set_measure: symmetric,
 *       NaN when min(e_a, e_b) == 0, exactly 1.0 on the diagonal of a self matrix.
 *     No clamp: estimator noise may put a containment below 0 or above 1.  These three work and are refused wherever JACCARD is.
 *     Two more measures read the OTHER sketch of every genome, its m SuperMinHash buckets (aux, u64 [n][m]; components (j << 32) | r):
 *       c(a, b) = #{ j < m : aux_a[j] == aux_b[j] }, compared on the full 64 bits -- buckets that differ in one dword only are unequal;
 *       SELHIP_MEASURE_SMH_MATCHES stores c as a number (0, 1, ..., m); SELHIP_MEASURE_SMH_JACCARD stores (double)c / (double)m, the
 *       SuperMinHash estimate of J (what `mash triangle` prints from such sketches).  Both are exact in SELHIP_F64 and, for c, in SELHIP_F32.
 *     No case is special: the diagonal of a self matrix is m (1.0), two empty sketches -- every bucket UINT64_MAX -- give m (1.0) as
 *     well, and the matrix is bit-symmetric.  These measures need the bucket rows alone (for a query matrix the queries' too, same m):
 *     any m > 0 and any p_hll that upload / attach accept, bit planes or none; aux is read in place, as uploaded or attached.
 *     Everything below holds for them unchanged, except the p_hll = 14 rule and the timer name ("matrix_smh").
 *     selhip_ctx_matrix: rows [r0, r1) of the context's sketches against all n of them; selhip_ctx_query_matrix: rows [r0, r1) of the
 *     attached queries (section 2b) against the n sketches of the database.  Ranks are those of the sets as uploaded (the cells do
 *     not depend on the order).
 *     out_dev: the caller's device buffer of out_rows x ld elements of dtype (aligned to the element), ld >= out_cols counted in
 *     elements.  row_pos / col_pos are HOST int32 arrays or NULL: the cell of rank-row i and rank-column k goes to
 *     out[row_pos[i]][col_pos[k]]; row_pos is indexed by rank and read for the ranks in [r0, r1) only, col_pos for all n columns;
 *     NULL = row_pos[i] = i - r0, col_pos[k] = k.  Passing the inverse of a sort permutation as both gives the matrix in the
 *     caller's original order without a gather.  Every position (the defaults too) is checked on the host before anything is
 *     launched -- 0 <= row position < out_rows, 0 <= column position < out_cols, SELHIP_E_BADARG with the first offending index in
 *     the message -- and only the checked copies reach the device.  Two rows (columns) sent to the same position is not an error:
 *     which one lands there is unspecified.  Cells of out_dev that no (row, column) of the call maps to are not written.
 *     SELHIP_E_BADARG also for: ld < out_cols, r0 > r1 or a range outside the set, a NULL or misaligned out_dev with cells to write, an
 *     unknown measure or dtype, a query matrix without attached queries, and -- for the HLL measures, the rule of
 *     SELHIP_CRIT_NONE -- sketches with p_hll != 14 or without resident bit planes ("hist_algo" 0).  n == 0 or r0 == r1: SELHIP_OK, nothing is written
 *     (the arguments above are checked all the same, except that out_dev may then be NULL and no position is read).
 *     SELHIP_E_STATE while a pass is pending.
 *     The call runs on the context's stream and returns when the matrix is complete.  It leaves the result list, result_count, the
 *     statistics, the top-k settings and the signature cache as they were; a context that never calls it launches what it always did.
 *     Its one kernel is timed as "matrix" (selhip_ctx_kernel_ms: per matrix call; the passes' per-pass figures are not touched).
 * --------------------------------------------------------------------------------------------------- */
#define SELHIP_MEASURE_JACCARD  0
#define SELHIP_MEASURE_UNION    1
#define SELHIP_MEASURE_SMH_MATCHES 16
#define SELHIP_MEASURE_SMH_JACCARD 17
#define SELHIP_MEASURE_INTERSECTION    32
#define SELHIP_MEASURE_CONTAINMENT     33
#define SELHIP_MEASURE_MAX_CONTAINMENT 34   /* also a measure of the passes: selhip_ctx_set_measure */
#define SELHIP_F64              0
#define SELHIP_F32              1
int selhip_ctx_matrix(selhip_ctx* ctx, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev,
                      int64_t out_rows, int64_t out_cols, int64_t ld, const int32_t* row_pos, const int32_t* col_pos);
int selhip_ctx_query_matrix(selhip_ctx* ctx, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev,
                            int64_t out_rows, int64_t out_cols, int64_t ld, const int32_t* row_pos, const int32_t* col_pos);

/* ---------------------------------------------------------------------------------------------------
 * 2g. Single-linkage clusters of the result list: the connected components of the graph whose edges are the records a pass left in
 *     device memory, with one representative per component -- dereplication ("which genomes are the same thing at J >= 0.95, and
 *     which one do I keep"), binning, "how many groups are in this collection" -- without fetching the list.
 *     THE GRAPH: its vertices are the n ranks of the context's set; its edges are the records of the result list the context holds, as
 *     selhip_ctx_result_device exposes it, whose `jaccard` field (the pass's measure) is >= min_value, compared in f64.  -INFINITY
 *     takes every record, NaN is SELHIP_E_BADARG, any other value is legal: one pass at a low tau_f can be cut at several levels.
 *     Accepted lists: all-pairs passes under any criterion, mode, measure or estimator, and the one-launch small pass; the cut lists of
 *     selhip_ctx_set_allpairs_topk, with or without row rounds (the k-NN graph: its directed records are taken as undirected edges);
 *     pair-list passes.  SELHIP_E_STATE after a query pass (its ranks live in two index spaces), before any finished pass and while
 *     a pass is pending.  A matrix call in between changes nothing.
 *     OUTPUTS, each a pure function of the record list, min_value and rep_rule, bit for bit, whatever order the device worked in:
 *       d_label[g]         the smallest rank of g's component
 *       d_cluster[g]       its dense id in 0 .. C-1, the components numbered by ascending label
 *       d_degree[g]        the RECORDS of the graph in which g appears as i or k -- records, not distinct partners: after a plain
 *                          all-pairs pass that is the vertex degree; in a directed top-k list a mutual pair counts twice for both of
 *                          its genomes, and in a pair list an entry listed twice counts twice
 *       d_cluster_size[c]  members of cluster c          (the first C entries are written)
 *       d_cluster_rep[c]   its representative's rank      (the first C entries are written), chosen by rep_rule:
 *           SELHIP_REP_MAX_DEGREE  the member with the most records; ties go to the smaller rank
 *           SELHIP_REP_MIN_RANK    the label: the smallest genome (ranks ascend with the cardinality)
 *           SELHIP_REP_MAX_RANK    the largest sketch of the cluster
 *         a singleton represents itself with degree 0; any other rule: SELHIP_E_BADARG.
 *     Every array is the caller's device memory of n int32; any of the five pointers may be NULL (that output is not written, and
 *     nothing else of the caller's is); *n_clusters_out (may be NULL) receives C.  n == 0: C = 0.
 *     The call reads the list and writes only `out` and scratch the context owns: the list, selhip_ctx_result_count, the statistics,
 *     selhip_ctx_last_attempts, the top-k settings and the signature cache are as they were, and a context that never calls it launches
 *     what it always launched.  It runs on the context's stream and returns when the outputs are complete.  A list without records
 *     (n singletons) is one launch.  Timed as "cluster" in selhip_ctx_kernel_ms: per cluster call, counted apart from the passes as
 *     "matrix" is.  get_param "clusters_last": the C of the last call, -1 = none yet.
 *     Not clustered: the host-side lists of selhip_multi_select and selhip_ooc_select (selhip_components takes any edge list).
 * --------------------------------------------------------------------------------------------------- */
#define SELHIP_REP_MAX_DEGREE 0
#define SELHIP_REP_MIN_RANK   1
#define SELHIP_REP_MAX_RANK   2
typedef struct {
    int32_t* d_label;        /* [n]  smallest rank of the genome's component                       */
    int32_t* d_cluster;      /* [n]  dense id 0 .. C-1, numbered by ascending label                */
    int32_t* d_degree;       /* [n]  records of the graph in which the genome appears as i or k    */
    int32_t* d_cluster_size; /* [n]  first C entries written: members of cluster c                 */
    int32_t* d_cluster_rep;  /* [n]  first C entries written: representative rank of cluster c     */
} selhip_clusters_t;         /* caller's device memory; any pointer may be NULL (not written)      */
int selhip_ctx_cluster(selhip_ctx* ctx, double min_value, int rep_rule,
                       const selhip_clusters_t* out, int64_t* n_clusters_out);

/* ---------------------------------------------------------------------------------------------------
 * 2h. Greedy representative clusters of the result list: the CD-HIT / UCLUST scheme, the one dereplication tools use to choose
 *     representatives.  Single linkage (2g) chains: with records A-B and B-C and none for A-C all three share a cluster, whose
 *     representative may have no record with some member at all.  Here every member is within min_value of ITS OWN representative,
 *     and no two representatives are within min_value of each other.
 *     THE GRAPH: the vertices are the n ranks of the context's set; the edges are the records of the result list with
 *     `jaccard` >= min_value in f64 and i != k.  -INFINITY takes every record, NaN min_value is SELHIP_E_BADARG, a NaN value is never an
 *     edge.  Repeated records, and the two directed records of a top-k list, are ONE edge; its value is the greatest of theirs.
 *     THE ORDER: every vertex has a 64-bit key and a greater key is visited first; keys are distinct, each ends in the reversed rank
 *       SELHIP_REP_MAX_DEGREE  (degree, reversed rank): the best connected first, ties to the smaller rank; degree as d_degree counts
 *       SELHIP_REP_MIN_RANK    reversed rank: the smallest genome first
 *       SELHIP_REP_MAX_RANK    rank: the largest sketch first, the CD-HIT order
 *       SELHIP_REP_PRIORITY    (d_priority[g], reversed rank): d_priority is the caller's uint32_t[n] in device memory, a quality score
 *                              for example; accepted by this entry only.  d_priority NULL with this rule (unless the context holds
 *                              an empty set: there is no score to read), or non-NULL with another rule, is SELHIP_E_BADARG; so is
 *                              any other rule.
 *     THE REPRESENTATIVES: visit the vertices by descending key; a vertex is a representative if and only if none of its neighbours is
 *     one already -- the lexicographically first maximal independent set of the graph under the order.  A vertex without an edge is one.
 *     THE ASSIGNMENT: every other vertex g belongs to the representative r for which the edge {g, r} has the greatest value; values
 *     compare as f64 (-0.0 equals +0.0), ties go to the smaller rank r.  A member's best edge to a NON-representative assigns nothing.
 *     OUTPUTS, each a pure function of the record list, min_value, the rule and d_priority, bit for bit, whatever order the device
 *     worked in:
 *       d_rep_of[g]        g's representative; a representative has itself
 *       d_value[g]         the value of the edge {g, d_rep_of[g]} with the record's bits (a zero of either sign is written +0.0);
 *                          1.0 for a representative
 *       d_cluster[g]       the dense id in 0 .. C-1 of g's cluster, the clusters numbered by ascending representative rank
 *       d_degree[g]        the RECORDS with `jaccard` >= min_value in which g appears as i or k, exactly as in 2g -- records, not
 *                          distinct partners, and a record with i == k counts twice for its genome though it is no edge
 *       d_cluster_size[c]  members of cluster c, the representative included   (the first C entries are written)
 *       d_cluster_rep[c]   its representative's rank                           (the first C entries are written)
 *     Every array is the caller's device memory of n elements; any of the six pointers may be NULL (that output is not written, and the
 *     launches that only serve it are skipped); *n_clusters_out (may be NULL) receives C.  n == 0: C = 0.
 *     Accepted lists and SELHIP_E_STATE cases: those of 2g (not after a query pass, not before any finished pass, not while a pass is
 *     pending).  The call reads the list and writes only `out` and scratch the context owns: the list, selhip_ctx_result_count, the
 *     statistics, selhip_ctx_last_attempts, the top-k settings, the signature cache and "clusters_last" are as they were, and a context
 *     that never calls it launches what it always launched.  It runs on the context's stream and returns when the outputs are complete.
 *     HOW (csrc/kernel_greedy.cuh): rounds of one launch over the records and one over the vertices -- a vertex none of whose earlier
 *     neighbours is undecided or a representative becomes one, a vertex behind a representative a member -- until a device counter
 *     reads no undecided vertex; no kernel waits for another lane.  Sparse lists take about ten rounds; a path whose keys ascend along
 *     it takes one round per vertex (short launches).  get_param "greedy_rounds_last": the first round after which no vertex was
 *     undecided (a list without records: 1; n == 0: 0); "greedy_clusters_last": C; both -1 = none yet.  Timed as "greedy" in
 *     selhip_ctx_kernel_ms: per greedy call, counted apart from the passes as "cluster" is.
 *     Not built: query passes, the host-side lists of selhip_multi_select and selhip_ooc_select (selhip_greedy_representatives takes
 *     any edge list), re-clustering of members around new centroids, distinct-partner degrees.  (For average or complete linkage
 *     see section 2k, over the dense matrix.)
 * --------------------------------------------------------------------------------------------------- */
#define SELHIP_REP_PRIORITY 3
typedef struct {
    int32_t* d_rep_of;       /* [n]  the genome's representative (itself for a representative)      */
    double*  d_value;        /* [n]  value of the edge to it; 1.0 for a representative              */
    int32_t* d_cluster;      /* [n]  dense id 0 .. C-1, numbered by ascending representative rank   */
    int32_t* d_degree;       /* [n]  records of the graph in which the genome appears as i or k     */
    int32_t* d_cluster_size; /* [n]  first C entries written: members of cluster c                  */
    int32_t* d_cluster_rep;  /* [n]  first C entries written: representative rank of cluster c      */
} selhip_greedy_t;           /* caller's device memory; any pointer may be NULL (not written)       */
int selhip_ctx_cluster_greedy(selhip_ctx* ctx, double min_value, int order_rule, const uint32_t* d_priority,
                              const selhip_greedy_t* out, int64_t* n_clusters_out);

/* ---------------------------------------------------------------------------------------------------
 * 2i. Sketches merged by group: one union sketch per cluster.  2g and 2h end in a dense cluster id per genome; this turns the ids
 *     into one sketch set per cluster -- a pan-genome sketch per species cluster, a sketch per metagenome bin, the first level of a
 *     two-level search -- without the rows leaving the device.
 *     THE IDENTITIES, both exact: the HLL sketch of a union of k-mer sets is the element-wise MAXIMUM of the registers (index and
 *     rank are functions of the hash alone; main and auxiliary sketches alike), its SuperMinHash sketch the element-wise unsigned
 *     MINIMUM of the 64-bit buckets (a bucket is the minimum over all elements and steps; an empty bucket stays ~0).  A merged row is
 *     bit for bit the row the sketch builder writes for the members' records concatenated.
 *     d_group[g] (device memory, int32[n], rank order) is the group of genome g, -1 .. n_groups - 1; -1 = in no group.  The d_cluster
 *     of selhip_ctx_cluster or selhip_ctx_cluster_greedy, with their C as n_groups, is a valid d_group as it is.
 *     OUTPUTS, n_groups rows in group-id order, each a pure function of the context's set and d_group, whatever order the device worked in:
 *       d_hll[c]      [1 << p_hll] u8   maximum of the members' main registers           (16-byte aligned)
 *       d_aux[c]      [m] u64           minimum of the members' SuperMinHash buckets     (8-byte aligned; 16 takes the wide path)
 *       d_aux_hll[c]  [1 << p_aux] u8   maximum of the members' auxiliary registers      (16-byte aligned); only where the context holds
 *                                       auxiliary sketches (uploaded, attached or folded): SELHIP_E_STATE otherwise
 *       d_cards[c]    f64               report() of the merged main registers: the kernels behind selhip_hll_cards, the context's fp mode
 *       d_size[c]     int32             members of group c
 *     An empty group: registers 0, buckets ~0, size 0, cardinality 0.  Every array is the caller's device memory; any of the five
 *     pointers may be NULL (that output is not written).  An id outside [-1, n_groups): SELHIP_E_BADARG, the message gives the number
 *     of such entries and the index of one of them, no output is written and no kernel reads or writes outside the arrays because of
 *     it.  n_groups == 0 writes nothing; a set of 0 genomes gives n_groups empty groups.  0 <= n_groups <= 2^31 - 1.
 *     SELHIP_E_STATE before upload / attach and while a pass is pending.  Allowed after any pass, a query pass included: it merges the
 *     database set.  The call writes only `out` and scratch the context owns: the result list, the statistics,
 *     selhip_ctx_last_attempts, the top-k settings, the signature cache and "clusters_last" are as they were.  It runs on the
 *     context's stream and returns when the outputs are complete.  Timed as "merge" in selhip_ctx_kernel_ms: per merge call, counted
 *     apart from the passes as "cluster" is.
 *     HOW (csrc/kernel_merge.cuh): a counting sort of the members by group, then a segmented reduction -- a lane per 16 bytes of an
 *     output row.  No lane reduces more than SELHIP_MERGE_SEGMENT rows: a longer group is first reduced to partial rows in scratch
 *     (ceil(size / SELHIP_MERGE_SEGMENT) of them), which the same kernel reduces again.
 *     Not built: merging query sets, the host-side lists of selhip_multi_select and selhip_ooc_select (selhost_merge_sketches serves
 *     them), intersections or differences of sketches, re-clustering around the merged rows.
 * --------------------------------------------------------------------------------------------------- */
#ifndef SELHIP_MERGE_SEGMENT
#define SELHIP_MERGE_SEGMENT 64      /* member rows one lane reduces at most (a group beyond it takes one more level per factor) */
#endif
typedef struct {
    uint8_t*  d_hll;         /* [n_groups][1 << p_hll]  merged main registers                        */
    uint64_t* d_aux;         /* [n_groups][m]           merged SuperMinHash buckets                  */
    uint8_t*  d_aux_hll;     /* [n_groups][1 << p_aux]  merged auxiliary registers                   */
    double*   d_cards;       /* [n_groups]              report() of the merged main registers        */
    int32_t*  d_size;        /* [n_groups]              members of the group                         */
} selhip_merged_t;           /* caller's device memory; any pointer may be NULL (not written)        */
int selhip_ctx_merge_groups(selhip_ctx* ctx, const int32_t* d_group, int64_t n_groups, const selhip_merged_t* out);

/* ---------------------------------------------------------------------------------------------------
 * 2j. Single-linkage hierarchy of the result list: the maximum spanning forest of the record graph.  2g answers one cut per call;
 *     the forest answers every cut at once.  Its F = n - C edges, best first, are the merge sequence of the single-linkage
 *     dendrogram; the clusters at any threshold t are the components of the forest edges with value >= t, and their number is n minus
 *     the number of such edges.  n - 1 records at the most, whatever the length of the list.
 *     THE GRAPH: the vertices are the n ranks of the context's set.  A record {i, k, value} of the result list is an edge if
 *     value >= min_value in f64 and i != k.  -INFINITY takes every record, NaN min_value is SELHIP_E_BADARG, a NaN value is never an
 *     edge.  The edge is the unordered pair {a, b}, a = min(i, k), b = max(i, k).  Repeated records of one pair, and the two directed
 *     records of a top-k list, are ONE edge; its value is the greatest of theirs, compared through the order-preserving integer image
 *     of section 2h's values, so -0.0 and +0.0 are one value, written +0.0.
 *     THE ORDER: edge e goes BEFORE edge f iff image(e.value) > image(f.value), or the images are equal and (e.a, e.b) is
 *     lexicographically smaller.  Distinct edges have distinct pairs: a strict total order.
 *     THE FOREST: visit the edges in that order and keep an edge iff its ends are not yet connected by kept edges (Kruskal).  Under a
 *     strict total order the result is unique.  It has F = n - C edges, C = selhip_ctx_cluster's C at the same min_value.
 *     OUTPUTS, each a pure function of the record list and min_value, bit for bit, whatever order the device worked in:
 *       d_edges[0 .. F)   selhip_pair_t {i = a, k = b, jaccard = value} in BEFORE order, best first: the caller's device memory of
 *                         max(n - 1, 0) records, 16-byte aligned (SELHIP_E_BADARG otherwise); entries from F on are not written
 *       d_label[g]        the smallest rank of g's component: selhip_ctx_cluster's d_label at the same min_value
 *       *n_edges_out      F (may be NULL)
 *     Either pointer may be NULL (not written); the struct may not.  n == 0 writes nothing.
 *     Accepted lists and SELHIP_E_STATE cases: those of 2g (not after a query pass, not before any finished pass, not while a pass is
 *     pending).  The call reads the list and writes only `out` and scratch the context owns: the list, selhip_ctx_result_count, the
 *     statistics, selhip_ctx_last_attempts, the top-k settings, the signature cache, "clusters_last" and "greedy_*_last" are as they
 *     were, and a context that never calls it launches what it always launched.  It runs on the context's stream and returns when the
 *     outputs are complete.
 *     HOW (csrc/kernel_forest.cuh): Boruvka rounds over the union-find of 2g.  A round is two launches over the records -- every
 *     component's best outgoing value by a 64-bit atomic maximum, then the smallest pair among the records of that value by an atomic
 *     minimum -- one over the vertices that emits each picked edge once and unites the two components, and one that flattens the
 *     components and counts the picks; a round that picks nothing ends the call: at most ceil(log2 n) + 1 rounds.  The emitted
 *     records are then sorted into BEFORE order (rocPRIM).  No kernel waits for another lane.  A list without records is one launch
 *     (F = 0, the identity labels).  get_param "forest_rounds_last": the rounds, the empty one included (a list without records: 1;
 *     n == 0: 0); "forest_edges_last": F; both -1 = none yet.  Timed as "forest" in selhip_ctx_kernel_ms: per forest call, counted
 *     apart from the passes as "cluster" is.
 *     Not built: query passes, the host-side lists of selhip_multi_select and
 *     selhip_ooc_select (selhip_spanning_forest takes any edge list), dropping the records inside one component between the rounds.
 *     (A Newick tree, and the hierarchy under the other linkages: section 2k.)
 * --------------------------------------------------------------------------------------------------- */
typedef struct {
    selhip_pair_t* d_edges;  /* [max(n-1,0)]  first F written: {a < b, value}, best first           */
    int32_t*       d_label;  /* [n]  smallest rank of the genome's component                        */
} selhip_forest_t;           /* caller's device memory; either pointer may be NULL (not written)    */
int selhip_ctx_spanning_forest(selhip_ctx* ctx, double min_value, const selhip_forest_t* out, int64_t* n_edges_out);

/* ---------------------------------------------------------------------------------------------------
 * 2k. Agglomerative hierarchy of the DENSE matrix: single, complete, average (UPGMA) and weighted (WPGMA) linkage, on the device.
 *     2g, 2h and 2j read the sparse record list; this call reads the n x n matrix of section 2f, turned into distances, and gives the
 *     dendrogram scipy.cluster.hierarchy.linkage gives for it (dRep's primary clustering, a tree from a `mash triangle`).
 *     THE SCHEME.  All four linkages are reducible -- d(i u j, k) >= min(d(i, k), d(j, k)) -- so every pair of RECIPROCAL NEAREST
 *     NEIGHBOURS can be merged at once and the dendrogram is the sequential algorithm's.  A round merges many pairs.
 *     STATE.  D: n x n f64, bit-symmetric; active[s], size[s] per slot s; a cluster lives in the slot of its smallest member; the
 *     nearest-neighbour cache nn[s], nd[s] and a dirty mark per slot.  At the start every slot is active, of size 1 and dirty.
 *     INPUT.  Only the strict upper triangle (a < b) is read; it is mirrored into the lower one first and the diagonal is ignored.  A
 *     NaN or -inf cell there: SELHIP_E_BADARG, the message gives the number of such cells and the indices of one, no output is
 *     written.  +inf is legal.
 *     A ROUND.
 *       1. Scan.  Every active dirty row r: nn[r] = the active slot b != r with the smallest D[r][b] under f64 `<`; equal values,
 *          -0.0 against +0.0 included, go to the smaller slot; nd[r] = D[r][nn[r]] with its bits.  All dirty marks are cleared.
 *       2. Pair.  P = {(a, b): a < b, both active, nn[a] == b, nn[b] == a, nd[a] <= max_height}.  P empty and every active row
 *          scanned in this very round: the call ends.  P empty otherwise (a RESCAN round: caches stale through ties or an ulp of
 *          rounding): every active row is marked dirty and the next round starts.  At most 2 (n - 1) + 1 rounds.
 *       3. Update.  LW(x, y, sa, sb) = min(x, y) single | max(x, y) complete | (sa * x + sb * y) / (sa + sb) average |
 *          0.5 * x + 0.5 * y weighted, in f64 with the sizes as doubles and EVERY product, sum and quotient rounded on its own (no
 *          fused multiply-add).  For a pair (a, b) of sizes sa, sb and a surviving slot k in no pair: v = LW(D[a][k], D[b][k], sa, sb).
 *          For two pairs (a, b), (c, d), a < c: v = LW(LW(D[a][c], D[a][d], sc, sd), LW(D[b][c], D[b][d], sc, sd), sa, sb).  v is
 *          stored at [a][k] and [k][a] (k = c in the second case).  All reads are of the matrix before the round.
 *       4. Record.  For every pair in ascending a: the merge {i = a, k = b, jaccard = nd[a]} and the size sa + sb are emitted;
 *          size[a] += size[b], b becomes inactive, a dirty; every active row whose cached nn is an a or a b of the round becomes dirty.
 *     OUTPUTS, each a pure function of the upper triangle, the method and max_height, bit for bit, whatever order the device worked in:
 *       d_merges[0 .. F)  the records in round order, ascending a within a round (children before parents): the caller's device
 *                         memory of max(n - 1, 0) records, 16-byte aligned (SELHIP_E_BADARG otherwise); entries from F on are not written
 *       d_size[0 .. F)    int32, the members of the cluster each merge made
 *       *n_merges_out     F <= n - 1; with max_height = INFINITY F = n - 1
 *     A cut at height h is selhip_components over the merges with value <= h; its labels go into selhip_ctx_merge_groups.
 *     selhip_ctx_linkage: measure = SELHIP_MEASURE_JACCARD, _MAX_CONTAINMENT or _SMH_JACCARD (the symmetric similarities; any other:
 *     SELHIP_E_BADARG); method = SELHIP_LINKAGE_*; a NaN max_height: SELHIP_E_BADARG.  The call takes n * n f64 of scratch
 *     (SELHIP_E_NOMEM if that cannot be had; released before it returns), fills it with the matrix kernels of 2f in rank order, turns
 *     every cell into the distance 1 - v (a NaN, which two empty sketches give under the HLL measures, into 1.0) and runs the rounds.
 *     What a matrix call refuses is refused here (p_hll != 14 or no bit planes for the HLL measures, a pending pass), and everything a
 *     matrix call leaves unchanged is left unchanged.  Timed as "linkage", per linkage call; "matrix" and "matrix_smh" are not touched.
 *     STREAM.  Every launch and copy of the call -- the matrix kernels, the distance kernel, each round's kernels, the small copies
 *     the host reads between the rounds, the copies into `out` -- runs on the context's stream (selhip_ctx_set_stream), in stream
 *     order behind whatever the caller put there: `out` may have been written on that stream right before the call.  The host waits
 *     for the stream after the matrix and twice per merging round, and the call returns when the outputs are complete: they may then
 *     be read from any stream.  Its scratch is taken and released inside the call, and releasing device memory waits for the whole
 *     device (see selhip_ctx_set_stream).
 *     get_param "linkage_rounds_last" (the rounds, rescan rounds and the empty last one included; n == 1: 1, n == 0: 0),
 *     "linkage_merges_last" (F), "linkage_rowscans_last" (rows scanned over all rounds), "linkage_rescans_last"; each -1 = none yet.
 *     HOW (csrc/kernel_linkage.cuh): the dirty rows are a device list; a workgroup per listed row streams it with 16-byte loads and
 *     reduces (value, slot) in the wave, then across the waves through LDS; one workgroup flags the pairs and compacts them in
 *     ascending order; one work item per (pair, column) updates in place; one lane per slot books sizes and the next list.  The host
 *     reads two words per merging round.  No kernel waits for another lane.
 *     Not built: Ward and centroid linkage, a condensed (triangular) matrix, matrices beyond device memory, query sets, a clusters
 *     table from the command line (it writes the tree and the merges: selection -N / -J), more than one device.
 * --------------------------------------------------------------------------------------------------- */
#define SELHIP_LINKAGE_SINGLE    0
#define SELHIP_LINKAGE_COMPLETE  1
#define SELHIP_LINKAGE_AVERAGE   2
#define SELHIP_LINKAGE_WEIGHTED  3
typedef struct {
    selhip_pair_t* d_merges; /* [max(n-1,0)]  first F written: {a < b, height}, in emitted order      */
    int32_t*       d_size;   /* [max(n-1,0)]  first F written: members of the merged cluster          */
} selhip_linkage_t;          /* caller's device memory; either pointer may be NULL (not written)    */
int selhip_ctx_linkage(selhip_ctx* ctx, int measure, int method, double max_height, const selhip_linkage_t* out, int64_t* n_merges_out);


/* ---------------------------------------------------------------------------------------------------
 * 3. Building blocks (device pointers), used by the launchers above and exposed for tests.
 * --------------------------------------------------------------------------------------------------- */
/* smh_a on an explicit pair list: d_flags[j] = 1 iff pair j has a fully equal band. */
int selhip_smh_a_pairs(const uint64_t* d_aux, int m, int n_rows, int n_bands,
                       const selhip_int2_t* d_pairs, int64_t n_pairs, uint8_t* d_flags, void* hip_stream);
/* union histogram of an explicit pair list: d_counts[j][64] (u32) = counts of max(reg_x, reg_y). */
int selhip_hll_union_hist(const uint8_t* d_hll, int p, const selhip_int2_t* d_pairs, int64_t n_pairs,
                          uint32_t* d_counts, void* hip_stream);
/* The p = 14 registers of n genomes as bit planes, the layout stage 2a reads (csrc/kernel_hllbs.cuh): d_planes[n][6][512] u32,
 * plane b of a genome = bit b of its 16 384 registers; d_gmax[n] u8 = every genome's largest register value; *khi_out = the
 * set's largest register value + 1.  Waits for the stream. */
int selhip_hll_bitslice(const uint8_t* d_hll, int64_t n_genomes, uint32_t* d_planes, uint8_t* d_gmax, int* khi_out, void* hip_stream);
/* union histograms from the bit planes (same result as selhip_hll_union_hist with p = 14); gmax / khi as returned above.  Waits. */
int selhip_hll_union_hist_planes(const uint32_t* d_planes, const uint8_t* d_gmax, int khi, const selhip_int2_t* d_pairs, int64_t n_pairs,
                                 uint32_t* d_counts, void* hip_stream);
/* Ertl-MLE of n histograms: d_est[j] = ertl_ml_estimate(d_counts[j], p, 64-p, 1e-2). */
int selhip_ertl_estimate(const uint32_t* d_counts, int64_t n, int p, int fp_mode, double* d_est, void* hip_stream);
/* bucket-match counts of an explicit pair list, one lane per pair: d_matches[j] = #{b : aux_x[b]==aux_y[b]}.  The same count of EVERY
 * pair as a dense array is SELHIP_MEASURE_SMH_MATCHES of section 2f; this entry stays as the independent check of it. */
int selhip_smh_match_counts(const uint64_t* d_aux, int m, const selhip_int2_t* d_pairs, int64_t n_pairs,
                            int32_t* d_matches, void* hip_stream);
/* HLL sketches of precision p folded to the lower precision p_aux: d_out[n][1 << p_aux] u8 from d_hll[n][1 << p] u8 (csrc/hll_fold.hpp,
 * csrc/kernel_fold.cuh).  With d = p - p_aux,
 *   out[g] = max over t in [0, 2^d) with r = in[(g << d) | t], r != 0 of ( t == 0 ? d + r : d - floor(log2 t) )      (0 if every r is 0)
 * which is the sketch the reference's hll_t (hll.h:886-888) builds at p_aux from the same hashes, bit for bit -- the .hll_<p_aux> file
 * beside a .hll file.  p in 4 .. 20, p_aux in 4 .. min(p, 15) (p_aux == p copies); SELHIP_E_BADARG outside, for a negative n, and with
 * n > 0 for a null pointer or one that is not 16-byte aligned.  n == 0 launches nothing.  Registers above 64 - p + 1 cannot come from
 * a sketch builder: what they fold to is unspecified, and nothing validates them.  Asynchronous on hip_stream. */
int selhip_hll_fold(const uint8_t* d_hll, int64_t n_genomes, int p, int p_aux, uint8_t* d_out, void* hip_stream);
/* Connected components of an edge list (csrc/kernel_cluster.cuh: a lock-free union-find, one lane per entry): d_label[g] = the smallest
 * vertex of g's component in the undirected graph on the vertices 0 .. n - 1 with one edge {x, y} per entry of d_pairs (device memory,
 * 8-byte aligned).  Entries with x == y and entries listed twice are legal and change nothing.  An entry with a vertex outside [0, n)
 * makes the call return SELHIP_E_BADARG: the message gives the number of such entries and the index of one of them, the labels are not
 * written, and no kernel reads or writes outside the arrays because of it.  n == 0 and n_pairs == 0 are legal (n_pairs == 0: n
 * singletons); 0 <= n <= 2^31 - 1, n_pairs any int64 >= 0.  The labels depend on the edge set alone.  Waits for the stream. */
int selhip_components(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, int32_t* d_label /*[n]*/, void* hip_stream);
/* The representatives of the greedy clustering (section 2h; csrc/kernel_greedy.cuh) over an edge list: d_is_rep[g] = 1 where g is in the
 * lexicographically first maximal independent set of the undirected graph on the vertices 0 .. n - 1 with one edge {x, y} per entry of
 * d_pairs (device memory, 8-byte aligned), 0 elsewhere.  The vertices are visited by descending d_key[g] (device memory, uint64_t[n]);
 * equal keys: the smaller vertex goes first; NULL d_key: key = vertex.  Entries with x == y and entries listed twice are legal and change
 * nothing.  *rounds_out (may be NULL): the rounds the selection took, at most those of the scheme with every read stale
 * (n_pairs == 0: 1; n == 0: 0).  Arguments, ranges, the SELHIP_E_BADARG of an entry with a vertex outside [0, n) -- d_is_rep is not
 * written -- and the messages are those of selhip_components.  Waits for the stream. */
int selhip_greedy_representatives(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, const uint64_t* d_key /* [n] or NULL */,
                                  uint8_t* d_is_rep /* [n] */, int64_t* rounds_out /* may be NULL */, void* hip_stream);
/* The maximum spanning forest (section 2j; csrc/kernel_forest.cuh) of an edge list: the undirected graph on the vertices 0 .. n - 1 with
 * one entry {x, y} of d_pairs (device memory, 8-byte aligned) per record and d_values[e] (device memory, f64) as its value; NULL
 * d_values = every value 1.0, and the order is then the pair order.  An entry with a NaN value is no edge; entries with x == y and
 * repeated entries are legal (a repeated pair is one edge with the greatest of its values).  d_edges (max(n - 1, 0) records, 16-byte
 * aligned), d_label ([n]), *n_edges_out (F) and *rounds_out (the rounds, the empty one included; n_pairs == 0: 1; n == 0: 0) are
 * section 2j's; each may be NULL.  Ranges, the SELHIP_E_BADARG of an entry with a vertex outside [0, n) -- whatever its value, and
 * nothing is written -- and its message are those of selhip_components.  The call owns its scratch and waits for the stream. */
int selhip_spanning_forest(const selhip_int2_t* d_pairs, const double* d_values, int64_t n_pairs, int64_t n,
                           selhip_pair_t* d_edges /* [max(n-1,0)] */, int32_t* d_label /* [n] */, int64_t* n_edges_out, int64_t* rounds_out,
                           void* hip_stream);
/* The hierarchy of section 2k over a caller's distance matrix d_dist[n][ld] (device memory, f64, 8-byte aligned, ld >= n counted in
 * elements), which the call works on and CONSUMES: its contents afterwards are unspecified.  With an even ld and a 16-byte aligned
 * base the row scan takes 16-byte loads, otherwise 8-byte ones; the results are the same.  d_merges (max(n - 1, 0) records, 16-byte
 * aligned), d_size, *n_merges_out (F) and *rounds_out (the rounds, rescan rounds and the empty last one included; n == 1: 1, n == 0: 0)
 * are section 2k's; each may be NULL.  SELHIP_E_BADARG: an unknown method, a NaN max_height, n < 0 or > 2^31 - 1, ld < n, a NULL matrix
 * with n > 1, a misaligned pointer, and a NaN or -inf cell in the strict upper triangle (no output is written).  SELHIP_E_NOMEM: no
 * room for the per-slot scratch.  The call owns its scratch and waits for the stream: every launch and copy runs on hip_stream, in
 * stream order -- the matrix and the outputs may have been written on that stream right before the call, and are read and overwritten
 * behind those writes --, the host waits for the stream twice per merging round, and the call returns when the outputs are complete
 * (they may then be read from any stream).  Releasing the scratch at the end waits for the whole device. */
int selhip_linkage(double* d_dist, int64_t n, int64_t ld, int method, double max_height, selhip_pair_t* d_merges /* [max(n-1,0)] */,
                   int32_t* d_size /* [max(n-1,0)] */, int64_t* n_merges_out, int64_t* rounds_out, void* hip_stream);
/* Sketches merged by group (section 2i; csrc/kernel_merge.cuh) over a caller's rows: d_hll[n][1 << p] u8, d_smh[n][m] u64 and
 * d_aux_hll[n][1 << p_aux] u8 reduced to n_groups rows each -- maximum, unsigned minimum, maximum -- by d_group[n] (int32, -1 .. n_groups - 1,
 * -1 = in no group; ids in any order); d_size_out[n_groups] (int32, may be NULL) receives the members per group.  A sketch kind is
 * present when its input and its output pointer are both non-NULL and absent when both are NULL; exactly one of the two: SELHIP_E_BADARG.
 * ALIGNMENT: HLL and auxiliary arrays 16 bytes, SuperMinHash arrays 8 bytes (16-byte aligned arrays with an even m take the 16-byte
 * path, anything else the 8-byte one: m = 1 and odd m are legal), d_group and d_size_out 4 bytes; SELHIP_E_BADARG otherwise.  Also
 * SELHIP_E_BADARG: p outside 4 .. 20; with auxiliary rows p_aux outside 4 .. 20; with SuperMinHash rows m < 1; n or n_groups negative or
 * above 2^31 - 1; and an id outside [-1, n_groups): the message gives the number of such entries and the index of one of them, no output
 * is written, and no kernel reads or writes outside the arrays because of it.  The maximum is exact for every byte value 0 .. 255,
 * not only for legal ranks.  An empty group: registers 0, buckets ~0, size 0.  n == 0 writes n_groups empty groups; n_groups == 0
 * writes nothing.  The call owns its scratch and waits for the stream. */
int selhip_merge_sketches(const uint8_t* d_hll, const uint64_t* d_smh, const uint8_t* d_aux_hll, int64_t n, int p, int m, int p_aux,
                          const int32_t* d_group, int64_t n_groups, uint8_t* d_hll_out, uint64_t* d_smh_out, uint8_t* d_aux_out,
                          int32_t* d_size_out, void* hip_stream);

/* ---------------------------------------------------------------------------------------------------
 * 4. Synthetic sketches generated directly in HBM (csrc/synth.hpp; stands in for the FASTA->sketch
 *    rebuild of experiments/src/time_smh_cuda.cpp:181-211).  Output is in GENERATION order (not sorted).
 * --------------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t seed;
    int32_t  n_genomes, m, p_aux, cluster_size, mode;
    uint32_t n_sh_lo, n_sh_hi;
} selhip_synth_t;
int selhip_synth_generate(const selhip_synth_t* sp, int64_t g_begin, int64_t g_end,
                          uint8_t* d_hll /*[g_end-g_begin][16384]*/, uint64_t* d_aux /*[..][m]*/,
                          uint8_t* d_aux_hll /*[..][1<<p_aux] or NULL*/, void* hip_stream);
/* gather rows into rank order: dst[r] = src[perm[r]] for row_bytes-sized rows (device pointers) */
int selhip_permute_rows(const void* d_src, void* d_dst, const int32_t* d_perm, int64_t n_rows,
                        int64_t row_bytes, void* hip_stream);

/* ---------------------------------------------------------------------------------------------------
 * 4b. Sketch construction (the `build_sketch` step, src/build_sketch.cpp:26-151): canonical k-mers of every
 *     genome -> HLL p=14 registers, optional auxiliary HLL (p_aux) and optional SuperMinHash h_[m], byte-identical
 *     to the files the reference writes.  d_codes: one byte per base (0..3 = A,C,G,T; 4 = window reset: non-ACGT
 *     character or record boundary), genomes concatenated; d_offsets[n_genomes+1] (int64) delimit them
 *     (selhost_fasta_codes produces the codes).  d_smh / d_aux_hll may be NULL.  m must already be rounded up to a
 *     power of two (policy.h:12-19), m <= 2048.  One workgroup per genome (selhip_build_sketches) or per chunk of a long
 *     genome (selhip_build_sketches_split).
 * --------------------------------------------------------------------------------------------------- */
int selhip_build_sketches(const uint8_t* d_codes, const int64_t* d_offsets, int64_t n_genomes, int k, int m, int p_aux,
                          uint8_t* d_hll, uint64_t* d_smh, uint8_t* d_aux_hll, void* hip_stream);
/* The same sketches with long genomes SPLIT across workgroups (csrc/kernel_sketch.cuh): byte for byte the rows
 * selhip_build_sketches writes.  The k-mer end positions of a genome of L codes are [k-1, L); with a chunk length C, chunk c owns the
 * end positions [k-1 + c C, min(k-1 + (c+1) C, L)); a genome has max(1, ceil((L - (k-1)) / C)) chunks and is split when it has two or
 * more.  Every chunk of a split genome is sketched by its own workgroup (pass 0: registers and step-0 offers) into scratch, the rows of
 * a genome are reduced as selhip_merge_sketches reduces a group (no lane reduces more than SELHIP_MERGE_SEGMENT rows in sequence), and a
 * split genome whose merged buckets show that pass 0 was not final (poly-A, mostly resets, fewer distinct k-mers than buckets) is
 * rebuilt whole by one more launch; every other genome is one workgroup, longest first.
 *   chunk: SELHIP_SPLIT_OFF (nothing is split), SELHIP_SPLIT_AUTO, or C itself, a positive multiple of 64.  AUTO never cuts below
 *     65 536 end positions: C = max(65 536, the call's end positions / (w x resident workgroups) rounded up to 65 536), w = 1, doubled
 *     until the partial rows (16 384 + 8 m + 2^p_aux bytes per chunk) fit 1 GiB.  An explicit C whose partial rows exceed 1 GiB:
 *     SELHIP_E_NOMEM with a message, nothing is written.
 *   h_offsets: the offsets on the host, or NULL: they are copied back from d_offsets once (not with SELHIP_SPLIT_OFF, which never reads them).
 *   A plan without a split genome (always with SELHIP_SPLIT_OFF; AUTO on short genomes; n_genomes == 0) issues exactly the launch of
 *   selhip_build_sketches.
 * SELHIP_E_BADARG before any HIP call, with a message and the outputs untouched: what selhip_build_sketches refuses; a chunk that is
 * none of the above; unless chunk is SELHIP_SPLIT_OFF, d_hll or d_aux_hll not 16-byte or d_smh not 8-byte aligned.  SELHIP_E_BADARG
 * before any launch, likewise: offsets (given on the host or copied back) that are negative or descend.  info (may be NULL) receives the plan and what ran: the chunk length (0: off),
 * the work items of the main launch, the split genomes and their chunks, the genomes rebuilt by the fallback launch, the levels of the
 * reduction (0 without a split genome) and the threads per workgroup of the main launch.  The call owns its scratch, works on the
 * caller's stream and waits for it. */
#define SELHIP_SPLIT_AUTO 0
#define SELHIP_SPLIT_OFF  (-1)
typedef struct { int64_t chunk, items, split_genomes, chunks, fallback_genomes; int32_t levels, threads; } selhip_build_info_t;
int selhip_build_sketches_split(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets /* or NULL: copied back once */,
                                int64_t n_genomes, int k, int m, int p_aux, int64_t chunk,
                                uint8_t* d_hll, uint64_t* d_smh, uint8_t* d_aux_hll, selhip_build_info_t* info /* or NULL */, void* hip_stream);
/* The plan of such a call as plain arithmetic; needs no device.  m, p_aux: of the rows the call would ask for (0: none), they size the
 * scratch; resident_blocks: the workgroups the device holds at once (what AUTO divides by; the entry above asks the runtime).
 * chunk_counts[n_genomes] (may be NULL) receives the chunks of every genome; info->chunk, items, split_genomes, chunks, levels and
 * threads are set, fallback_genomes is 0.  SELHIP_E_BADARG (bad chunk, k outside 1 .. 32, bad offsets) and SELHIP_E_NOMEM as above. */
int selhip_build_split_plan(const int64_t* h_offsets, int64_t n_genomes, int k, int m, int p_aux, int64_t chunk, int64_t resident_blocks,
                            int64_t* chunk_counts /* [n_genomes] or NULL */, selhip_build_info_t* info);

/* ---------------------------------------------------------------------------------------------------
 * 5. Plain device-memory helpers so that a host program needs no HIP headers (the reference driver
 *    calls cudaMalloc/cudaMemcpy/cudaFree directly, selection_cuda.cpp:160-182).
 * --------------------------------------------------------------------------------------------------- */
int selhip_malloc(void** d_ptr, size_t bytes);
int selhip_free(void* d_ptr);
int selhip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes);
int selhip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes);
int selhip_device_synchronize(void);

const char* selhip_version(void);

#ifdef __cplusplus
}
#endif
#endif /* SELECTION_HIP_H */

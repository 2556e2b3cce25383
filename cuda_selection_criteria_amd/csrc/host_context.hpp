// host_context.hpp -- the context of libselhip.so (struct selhip_ctx), its device buffers (DevBuf; SigSet, BitPlanes and CounterSets, one
// definition each for the database's, the queries' and the query passes' instances), kernel timers and small helpers.
// Part of the kernel translation unit selection_kernels.hip (included there, after the kernel headers); not a stand-alone header.
#pragma once

namespace {

// =============================================================================================
// host side
// =============================================================================================
thread_local std::string g_last_error = "";

void set_err(std::string* dst, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (dst) *dst = buf;
    g_last_error = buf;
}

#define HIPCHK(ctx_err, expr)                                                                  \
    do {                                                                                       \
        hipError_t e__ = (expr);                                                               \
        if (e__ != hipSuccess) {                                                               \
            set_err(ctx_err, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
            return SELHIP_E_HIP;                                                               \
        }                                                                                      \
    } while (0)

// a run-time flag that a kernel takes as a template argument (the estimator's SELHIP_FP_FMA mode above all): f(std::true_type{}) or
// f(std::false_type{}), so that the launch is written once -- with_flag(fma, [&](auto F) { ...kernel<decltype(F)::value>... })
template <typename F>
auto with_flag(bool flag, F&& f) { return flag ? f(std::true_type{}) : f(std::false_type{}); }

template <typename T>
struct DevBuf {
    T* p = nullptr;
    size_t cap = 0;   // elements
    hipError_t ensure(size_t n) {
        if (n <= cap) return hipSuccess;
        if (p) { (void)hipFree(p); p = nullptr; cap = 0; }
        hipError_t e = hipMalloc((void**)&p, n * sizeof(T));
        if (e == hipSuccess) cap = n;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
};

// the four layouts the signature builder writes for one sketch set: genome-major / band-major / band-major 16-bit pairs / genome-major
// 16-bit pairs (Q, T, P, G)
struct SigSet {
    DevBuf<uint32_t> Q, T, P, G;
    // room for n genomes of nb bands.  *moved (if asked for): an array was reallocated, so whatever a cache key says they hold is gone
    hipError_t ensure(size_t n, size_t nb, bool* moved = nullptr) {
        const uint32_t* const old[4] = {Q.p, T.p, P.p, G.p};
        const size_t n_pad = pad_wave(n), half = (nb + 1) / 2;
        hipError_t e = Q.ensure(std::max<size_t>(1, n * nb));
        if (e == hipSuccess) e = T.ensure(std::max<size_t>(1, n_pad * nb));
        if (e == hipSuccess) e = P.ensure(std::max<size_t>(1, n_pad * half));
        if (e == hipSuccess) e = G.ensure((n_pad + 2) * half);
        if (moved) *moved = Q.p != old[0] || T.p != old[1] || P.p != old[2] || G.p != old[3];
        return e;
    }
    void release() { Q.release(); T.release(); P.release(); G.release(); }
};

// writes the bit planes of n genomes and returns max register value + 1 through *khi (waits for the stream)
int build_bitslices(std::string* err, hipStream_t st, const uint8_t* d_hll, int64_t n, uint32_t* d_bs, uint8_t* d_gmax, int* d_max, int* khi) {
    HIPCHK(err, hipMemsetAsync(d_max, 0, sizeof(int), st));
    hipLaunchKernelGGL(hll_bitslice_kernel, dim3(grid_for((u64)n, kWavesPerBlock, 8192)), dim3(kBlock), 0, st, d_hll, (long long)n, d_bs, d_gmax, d_max);
    HIPCHK(err, hipGetLastError());
    int mx = 0;
    HIPCHK(err, hipMemcpyAsync(&mx, d_max, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    *khi = mx + 1;
    return SELHIP_OK;
}

// stage 2a on bit planes (kernel_hllbs.cuh): the p = 14 registers of every genome of a sketch set as 6 bit planes (12 KiB per genome;
// the byte rows stay for report() and the callers)
struct BitPlanes {
    DevBuf<uint32_t> bs;                // [n][6][512]
    DevBuf<uint8_t> gmax;               // [n] largest register value of each genome
    DevBuf<int> dev_max;                // largest register value of the set (device side)
    int khi = 0;                        // 0 = no planes; else max register value + 1
    int build(std::string* err, hipStream_t st, const uint8_t* d_hll, int64_t n) {
        HIPCHK(err, bs.ensure((size_t)n * kBsGenomeDwords));
        HIPCHK(err, gmax.ensure((size_t)n));
        HIPCHK(err, dev_max.ensure(1));
        return build_bitslices(err, st, d_hll, n, bs.p, gmax.p, dev_max.p, &khi);
    }
    void release() { bs.release(); gmax.release(); dev_max.release(); }
};

// scratch of a merge by group (kernel_merge.cuh, host_merge.hpp): selhip_ctx_merge_groups keeps one, selhip_merge_sketches owns one per call
struct MergeScratch {
    DevBuf<int> cnt, order;             // members per group (the scatter's cursors); the members in group order
    DevBuf<u64> pk;                     // a level's scan input
    DevBuf<u64> scan[kMergeMaxLevels];  // per level: member offset << 32 | output-row offset of every group, the totals in slot G
    DevBuf<char> tmp;                   // rocPRIM scan scratch
    DevBuf<uint4> part[2];              // partial rows of the levels before the last, ping-pong
    DevBuf<MergeInfo> info;
    void release() {
        cnt.release(); order.release(); pk.release(); tmp.release(); part[0].release(); part[1].release(); info.release();
        for (auto& s : scan) s.release();
    }
};

// scratch of the graph calls over the result list (host_graph.hpp), by role.  No call keeps anything in it: each ensures what it uses and initialises what it reads
struct GraphScratch {
    DevBuf<int> parent, label, degree, members;   // the union-find forest; labels, degrees, members per root or representative where the caller takes none
    DevBuf<int> state, blocked, rep_of; // greedy: UNDECIDED / REP / MEMBER; the last round a vertex was held back; rep_of where the caller takes none
    DevBuf<uint32_t> flag, ids, words;  // root / representative flags, their exclusive scan (one slot past the last genome: the number of clusters); the counters of a batch of rounds
    DevBuf<u64> key, best;              // representative key / greedy key / component's best image; a member's best image / a component's best pair
    DevBuf<ClusterBad> bad;             // records an edge kernel refused (none, unless a list is corrupt)
    DevBuf<char> tmp;                   // rocPRIM scan / sort scratch
    DevBuf<ForestEdge> edges;           // the forest's emitted records before their sort
    void release() { parent.release(); label.release(); degree.release(); members.release(); state.release(); blocked.release(); rep_of.release(); flag.release();
                     ids.release(); words.release(); key.release(); best.release(); bad.release(); tmp.release(); edges.release(); }
};

// TWO sets of per_set counter blocks: pass k uses set k & 1 and its first kernel clears the other for pass k + 1 -- no memset dispatch
// on the stream in steady state.  dirty: a pass claimed a set and did not get to the end of its enqueue (its first kernel may never have
// run), or nothing has cleared the buffer yet, or the stream changed behind the clearing: the next claim clears both sets first, once
struct CounterSets {
    DevBuf<PassCounters> buf;
    int per_set = 1, flip = 0;
    bool dirty = false;
    struct Claim { PassCounters* cur; PassCounters* next; };
    // the set of the pass being enqueued and the one its first kernel clears; the caller resets `dirty` when its enqueue is complete
    hipError_t claim(hipStream_t st, Claim* out) {
        if (dirty) {
            const hipError_t e = hipMemsetAsync(buf.p, 0, sizeof(PassCounters) * 2 * per_set, st);
            if (e != hipSuccess) return e;
        }
        *out = Claim{buf.p + (size_t)flip * per_set, buf.p + (size_t)(flip ^ 1) * per_set};
        flip ^= 1;
        dirty = true;
        return hipSuccess;
    }
};

struct KernelTimer {
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev;
    std::vector<long> ev_pass;          // the pass each pair was recorded in
    double total_ms = 0;
    double span_ms = 0;                 // per pass: first start -> last end (chunk lanes run a kernel's launches side by side)
    long launches = 0;
};

constexpr int kMaxChunks = 8;
constexpr size_t kSegCounterSlots = (size_t)(kMaxChunks + 1) * kAppendSegs * kSegStride;    // the join's append-segment counters (u64 slots)
// pairs per pass from which the automatic setting splits a pass into two chunk lanes (one MI355X, cfg3 data at growing genome counts,
// lanes off -> 2: 4.0e8 pairs 1.033 -> 1.034 ms, 5.4e8 1.319 -> 1.289, 7.2e8 1.648 -> 1.622, 1.0e9 2.290 -> 2.154; an eighth of cfg4's rows,
// 6.2e8 pairs, 0.446 -> 0.431 ms)
constexpr double kAutoChunkPairs = 5e8;
static_assert(kCounterBlocks == kMaxChunks + 1, "common.cuh: counter blocks per pass");
constexpr int kMaxAuxP = SELHIP_MAX_AUX_P;   // auxiliary HLL precision accepted by every entry point: aux_fused_kernel counts in 16-bit bins (a bin holds up to 2^p_aux)
constexpr long long kEnumPairs = 1ll << 26;    // hll_a / hll_an as first criterion: pairs listed per sub-pass (512 MiB of int2)

enum { T_PREP = 0, T_STAGE1, T_HIST, T_SELECT, T_TOTAL, T_SIGBUILD, T_JOIN, T_VERIFY, T_AUX, T_GROUP, T_DENSE, T_TOPK, T_MATRIX, T_MATRIX_SMH, T_CLUSTER, T_GREEDY, T_MERGE, T_FOREST, T_LINKAGE, T_COUNT };
const char* kTimerNames[T_COUNT] = {"prep", "stage1", "hist", "select", "total", "sigbuild", "join", "verify", "aux", "group", "dense", "topk", "matrix", "matrix_smh", "cluster", "greedy", "merge", "forest", "linkage"};

}  // namespace

struct selhip_ctx {
    int device = 0;
    int dev_cus = 0;                    // compute units of the device (the one-launch pass of a small set needs all 256 of an MI355X)
    hipStream_t stream = nullptr;
    int fp_mode = SELHIP_FP_FMA;
    std::string err;

    // sketches (owned or attached)
    bool owns_sketches = false;
    const uint8_t* d_hll = nullptr;
    const u64* d_aux = nullptr;
    const double* d_cards = nullptr;
    DevBuf<uint8_t> own_hll;
    DevBuf<u64> own_aux;
    DevBuf<double> own_cards;
    int64_t n = 0;
    int m = 0, p = 14;

    // derived / scratch
    DevBuf<u64> ecard;
    DevBuf<int> hi;
    CounterSets pc{{}, kMaxChunks + 1}; // kMaxChunks + 1 blocks per set; cleared once at allocation (ensure_scratch), so it starts clean
    PassCounters* pcb = nullptr;        // the set of the pass enqueued last
    int fail_after_flip = 0;            // test hook ("fail_after_flip"): the next enqueue returns an error right after claiming its counter set
    DevBuf<u64> seg_cnt;                // the join's append-segment counters: (kMaxChunks + 1) x kAppendSegs x kSegStride
    DevBuf<selhip_int2_t> surv;
    DevBuf<uint32_t> counts;
    DevBuf<selhip_pair_t> results;
    DevBuf<selhip_int2_t> self_pairs;
    DevBuf<selhip_int2_t> cand;         // ALGO_SIG: signature-join candidates; aux criteria: enumerated pairs
    DevBuf<selhip_int2_t> fin;          // aux criteria: pairs that passed hll_a / hll_an
    const uint8_t* d_aux_hll = nullptr; // auxiliary HLL registers [n][1 << p_aux]
    DevBuf<uint8_t> own_aux_hll;
    int p_aux = 0;
    int criterion = 0;
    DevBuf<u64> aux_il;                 // ALGO_STREAM: bucket-interleaved copy of the sketches (kernel_stream.cuh)
    SigSet sig;                         // ALGO_SIG: band signatures
    DevBuf<u64> hj_keys_in, hj_keys_out;   // ALGO_HASHJOIN: (band << 32 | signature) keys, before / after the sort
    DevBuf<int> hj_vals_in, hj_vals_out;   //                genome ranks carried by the keys
    DevBuf<char> hj_tmp;                   //                rocPRIM temporary storage
    DevBuf<int> csr_cnt, csr_start;        // stage 2 grouping: survivors per query row (cnt[0..n) counts, cnt[n..2n) fill cursors), offsets
    DevBuf<selhip_int2_t> grouped;         //                   the final pair list bucketed by query row
    DevBuf<char> scan_tmp;
    size_t scan_tmp_stride = 0;         // bytes of rocPRIM scan scratch per chunk
    PassCounters* h_pc = nullptr;       // pinned host mirror of the kMaxChunks + 1 counter blocks
    // stage pipeline: stage 1 of row chunk c+1 (VALU-bound) overlaps stage 2 of chunk c (memory/LDS-bound)
    hipStream_t st_stage1 = nullptr;    // internal non-blocking stream: the second chunk lane (the first is `stream`)
    hipEvent_t ev_start = nullptr, ev_end = nullptr;       // fork / join of the second lane
    int n_chunks_last = 1;
    int pipeline = -1;                  // -1 auto, 0 off, >0 forced chunk count
    int64_t cand_begin = 0;             // candidates restricted to ranks >= cand_begin (selhip_ctx_set_candidate_begin)
    int il_block = 128, il_parts = 1, il_part = 0;    // row interleave (selhip_ctx_set_row_interleave); il_parts 1 = contiguous
    int hist_pad = 0;                   // stage 2a: extra LDS bytes per one-wave block (lowers the number of resident waves per CU)
    int hist_run = 0, hist_blocks = kHistSpanBlocks;   // stage 2a: pairs per task (0 = automatic: 1, or 4 with the label order), one-wave blocks (multiple of 8)
    // the database's bit planes, written when the sketches are uploaded / attached (selhip_ctx_upload / _attach; the caller's arrays
    // must not change behind an attached context)
    BitPlanes planes;
    DevBuf<u64> small_bar;              // the one-launch pass's barrier: 16 group words, 128 bytes apart
    // sparse lists of every genome's registers >= hll_sparse_t ([n][kBsSparseCap], written with the planes): stage 2a decodes only the
    // values below the threshold from the planes.  hll_sparse_t = 0: no lists (the set needs a threshold above kBsSparseMaxT)
    DevBuf<uint32_t> hll_sparse;
    DevBuf<int> hll_sparse_dev_t;
    int hll_sparse_t = 0;
    int hist_sparse = -1;               // "hist_sparse": -1 automatic (sparse_t_used), 1 = use the lists where the set has them, 0 = every value from the planes
    // the clamped image of every genome ([n][4][512], min(register, 15) as four planes: kernel_hllbs.cuh), written with the lists where
    // hll_sparse_t <= kBsImageMaxT (hll_image_ok; every upload / attach clears it and rebuilds the image, a failed one leaves none): what
    // stage 2a reads in place of the planes wherever it takes the lists at such a threshold
    DevBuf<uint32_t> hll_image;
    bool hll_image_ok = false;
    int hist_image = -1;                // "hist_image": -1 automatic, 1 = the image wherever it is exact (the same today), 0 = the six-plane rows
    int hist_image_used = 0;            // the last all-pairs pass's stage 2a read the image (get_param "hist_image")
    int hist_algo = -1;                 // -1 automatic (bit planes when p = 14), 0 = byte rows + LDS histogram (hll_union_hist_runs_kernel), 1 = bit planes
    int hist_dense_degree = 32;         // bit-plane kernel: survivors per query row from which a grouped list is walked by candidate slice per XCD (-1 = never)
    int hist_bs_blocks = 2048;          // bit-plane kernel: 4-wave blocks (multiple of 8)
    int group_label = -1;               // grouping: lay the query-row buckets out by label (kernel_hll.cuh): -1 = automatic (HLL rows beyond kLabelOrderBytes), 0 off, 1 on
    int verify_fb = 0;                  // test hook: force the collision fallback of verify16_kernel
    int join_wpb = 4;                   // 16-bit join: waves per block (DPP form: 1 or 4; LDS form: 4 or 8 -- the waves of a block share the staged query tile)
    int join_db = 1;                    // 16-bit join: double-buffered query batches
    int join_tri = 0;                   // LDS-tile join: 1 = launch only the (tile, candidate block) units above the diagonal (measured: no gain, see JoinTriangle); 0 = the rectangle
    // 16-bit LDS-tile join, inner loop: 2 = bit-sliced signatures, one v_bitop3_b32 per dword (where the tiled build takes the band
    // shape; packed minimum otherwise), 0 = xor + v_pk_min_u16, 1 = zero-half test (xor, sub, v_bitop3_b32; measured slower, see kernel_sigjoin.cuh)
    int join_form = 2;
    int join_form_used = -1;            // kernel FORM of the last LDS-tile join launched (launch_joinl), -1 = none yet
    int join_t = 0;                     // sliced join: candidate groups of 64 per wave, 1 or 2 (2 only for nb <= 64); 0 = automatic (launch_joinl_f)
    int join_bits = 16;                 // signature width of the all-pairs join: 16 (packed min), 15 (LDS form only: flag arithmetic, all plain VOP2) or 32
    int join_q = 1;                     // 16-bit join, query side: 1 = tile staged in LDS, broadcast reads (sigl_join_kernel), 0 = DPP row broadcast (sig16_join_kernel)
    long long enum_pairs = kEnumPairs;  // hll_a / hll_an as first criterion: pairs listed per sub-pass (test hook "enum_pairs")
    // genomes per tile of the tiled signature build ("sig_tile_g": 8 / 16 / 32).  Measured, build alone, 8 / 16 / 32: cfg3 15.9 / 16.4 / 21.3 us,
    // 28 280 genomes 36.9 / 35.0 / 42.2, cfg4 64.5 / 60.4 / 67.2 (gpurun_out/r03/o_*): full 128-byte band-major segments (32) do not pay
    int sig_tile_g = 16;
    int sig_cache = 0;                  // keep the band signatures across passes ("sig_cache"); sig_key = what the arrays hold (0 = nothing)
    long long sig_key = 0;
    int sig_tile = 1;                   // signature build: tiled form (0 = one thread per bucket, the round-1 kernel)
    int init_cap = 0;                   // test hook: initial capacity of the survivor / candidate lists (0 = sized from the workload)
    int join_qt = 0;                    // query rows per signature-join block (multiple of 16); 0 = automatic: 32 rows below 1e8 pairs per pass, 64 up to 4.5e8
                                        // (30 000 genomes on one GPU; 2e8 since round 3), 128 beyond.  With the segmented appends: cfg3 112 / 114 / 127 us at 64 / 96 / 128 rows (finer tiles balance
                                        // the 1 024 SIMDs better), cfg4 2.12 / 2.10 / 2.07 ms (a block's prologue -- 32 candidate loads per lane,
                                        // tile staging -- is amortised over more rows), cfg5 8.31 / 8.16 / 8.20 ms
    bool group_stage2 = true;           // bucket survivors by query row before stage 2a (hll_union_hist_runs_kernel)
    int small_pass = -1;                // sets of <= 2 048 genomes: the whole pass in one cooperative launch (kernel_small.cuh); -1 automatic, 0 off
    bool small_used = false, small_pass_failed = false;   // the last enqueue took it / a block's survivor list overflowed once: regular passes from then on
    int group_min_n = 2048;             // ... for sets of more than this many genomes ("group_min_n"; see grouping_on)
    // SELHIP_CRIT_NONE ("dense_fused"): 1 = dense_select_kernel (kernel_dense.cuh), 0 = the list route (enumeration, then the union-histogram
    // and estimator kernels of the other criteria); dense_route_used = which the last such pass took (-1 = none yet)
    int dense_fused = 1;
    int dense_route_used = -1;
    // SELHIP_CRIT_SMH_C (kernel_smhc.cuh): the count threshold (selhip_ctx_set_min_matches; 0 = never set) and the stage-1 kernel of the
    // last such pass (1 the fast path, 0 the generic one, -1 none yet)
    int min_matches = 0;
    int smhc_path_used = -1;
    // its per-pair rule (selhip_ctx_set_min_containment; NaN = never set or cleared: the fixed rule) and the rule of the last such pass
    // (0 fixed, 1 containment, -1 none yet)
    double min_containment = std::numeric_limits<double>::quiet_NaN();
    int smhc_rule_used = -1;
    // what stage 2 of every pass tests against tau and records (selhip_ctx_set_measure): SELHIP_MEASURE_JACCARD or _MAX_CONTAINMENT
    int measure = SELHIP_MEASURE_JACCARD;
    // which estimate the records of an smh_c pass carry (selhip_ctx_set_estimator): SELHIP_ESTIMATOR_HLL, or _SMH -- stage 1 emits them
    int estimator = SELHIP_ESTIMATOR_HLL;

    // last run parameters (for overflow re-runs)
    bool have_run = false, pending = false;
    int mode = 0, algo = 0, n_rows = 0, n_bands = 0;
    PassPlan plan;                      // which stage 1 these parameters and the criterion select (pass_plan; set by run_async / run_queries)
    float tau_f = 0;
    int64_t row_begin = 0, row_end = 0;
    PassCounters last{};

    // query passes (abi_query.inc, host_query.hpp): a second sketch set Q, in its own buffers, matched against the sketches above (D)
    struct QuerySet {
        int64_t n = -1;                             // -1 = no queries loaded (uploading / attaching the database drops them)
        const uint8_t* d_hll = nullptr;
        const u64* d_aux = nullptr;
        const double* d_cards = nullptr;
        DevBuf<uint8_t> own_hll;
        DevBuf<u64> own_aux;
        DevBuf<double> own_cards;
        BitPlanes planes;                           // Q's bit planes, written at upload / attach
        DevBuf<int> lo, hi;                         // CB window of every query in D
        DevBuf<u64> ecard;                          // truncated cards, combined index space: [0, n) = Q, [n, n + n_D) = D
        SigSet sig;                                 // Q's band signatures (sig.Q is read; the builder writes all four layouts)
        SigSet db_sig;                              // D's band signatures, kept across query passes
        long long db_sig_key = 0;                   // (n_rows, n_bands, database generation) they were built for; 0 = none
        int db_sig_builds = 0;                      // builds of D's signatures since the database was loaded ("query_db_sig_builds")
        // ALGO_INDEX (kernel_query_index.cuh): per band, D's signatures sorted ascending and the database ranks they belong to
        // ([n_bands][n_D] each).  Buffers of its own: an all-pairs ALGO_HASHJOIN pass in between leaves it alone
        DevBuf<uint32_t> db_idx_sig;
        DevBuf<int> db_idx_rank;
        DevBuf<int> db_idx_dir;                     // bucket directory: [n_bands][2^db_idx_dir_bits + 1] offsets into a band's segment
        int db_idx_dir_bits = 0, db_idx_bands = 0;
        long long db_idx_key = 0;                   // as db_sig_key; 0 = none
        int db_idx_builds = 0;                      // index builds since the database was loaded ("query_db_index_builds")
        BitPlanes db_planes;                        // D's bit planes, only if the all-pairs path keeps none (hist_algo 0)
        long long db_bs_gen = -1;
        DevBuf<selhip_int2_t> cand, surv;
        DevBuf<selhip_int2_t> fin;                  // criteria other than smh_a: the pairs that passed hll_a / hll_an (stage 2's list)
        const uint8_t* d_aux_hll = nullptr;         // Q's auxiliary HLL registers [n][1 << p_aux] (dropped by every upload / attach of Q)
        DevBuf<uint8_t> own_aux_hll;
        int p_aux = 0;                              // 0 = none loaded
        DevBuf<uint32_t> counts;
        CounterSets pc{{}, 1, 0, true};             // one block per set; nothing clears it at allocation, so it starts dirty
        PassCounters* h_pc = nullptr;
    } q;
    long long db_gen = 0;               // incremented by every upload / attach of the database
    int query_index_dir = 1;            // ALGO_INDEX: the probe starts from the bucket directory (0 = searches the whole band segment; "query_index_dir")
    int query_join_tile = 16;           // queries per block of the query passes' signature join (16 or 32; "query_join_tile")
    bool last_was_query = false;        // the results / statistics held are those of a query pass (no framed copies of them)
    // top-k of the query passes (selhip_ctx_set_query_topk; kernel_topk.cuh, host_topk.hpp)
    int query_topk = 0;                 // K: every query keeps its K best records; 0 = off
    int allpairs_topk = 0;              // K of the all-pairs passes (selhip_ctx_set_allpairs_topk; kernel_topk.cuh, BOTH): every genome keeps its K best partners; 0 = off
    bool topk_applied = false;          // the result list holds topk(S, K) of the last finished query pass -- or nbr(S, K) of the last all-pairs pass --, in ranked order ...
    int64_t topk_n = 0;                 // ... and this many records (last.n_results stays |S|)
    DevBuf<uint32_t> topk_cnt;          // records per query, then the scatter's fill cursors
    DevBuf<u64> topk_off;               // scanned: (output start << 32) | segment start, one slot past the last query = the totals
    DevBuf<u64> topk_key;               // the records grouped by query: key(J) ...
    DevBuf<uint32_t> topk_val;          // ... and database rank
    DevBuf<char> topk_tmp;              // rocPRIM scan scratch
    // all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds): the pass runs as sub-range passes of `rows` rows,
    // each merged into the carried list C, whose K-th values are the next round's admission thresholds
    int64_t topk_rounds = 0;            // the setting: 0 = off, > 0 rows per round, SELHIP_TOPK_ROUNDS_AUTO = topk_round_rows' choice
    int rounds_used = 0;                // rounds of the last such pass ("topk_rounds_used") ...
    u64 rounds_admitted = 0;            // ... and the records its count kernels appended over all of them ("topk_admitted_lo" / "_hi")
    struct Rounds {                     // the pending pass
        bool on = false;                // run_async took the round route: [begin, end) below is the round enqueued, not the pass's rows
        int64_t rows = 0, begin = 0, end = 0;
        u64 n_carry = 0;                // |C|
        PassCounters acc{};             // the counters of the accepted rounds, added up
        int attempts = 0;               // the most enqueues any round needed
    } rd;
    DevBuf<selhip_pair_t> topk_carry;   // C: directed records {owner, partner, V} in ranked order; swapped with the result list behind the last round
    DevBuf<double> topk_thr;            // thr[n]

    // pair-list passes (selhip_ctx_run_pairs; abi_pairs.inc, host_pairs.hpp): the pending / last pass evaluates a caller's list
    bool list_pass = false;
    const selhip_int2_t* list_pairs = nullptr;     // the caller's, alive until selhip_ctx_finish (a pass that outgrows a list reads it again)
    int64_t list_n = 0;
    int pairs_route_used = -1;          // stage 1 of the last list pass: 1 signature route, 0 direct route, 2 no smh_a stage, -1 none yet
    int pairs_gpw_used = -1;            // ... its groups per wave (pairs_direct_shape; 0: a kernel of one lane per entry), -1 none yet
    int pairs_grid_used = -1;           // ... and the grid of its stage-1 kernel (criteria that take the list in windows: of the first), -1 none yet

    // dense matrices (selhip_ctx_matrix / _query_matrix; abi_matrix.inc): the validated copies of the caller's positions
    DevBuf<int> mat_row_pos, mat_col_pos;
    int matrix_mirror = 1;              // test switch ("matrix_mirror"): 0 = a self matrix stores no mirrored cells (upper triangle of a slab only)
    // the SuperMinHash measures (kernel_matrix_smh.cuh): "matrix_smh_form" 1 = a self matrix computes every pair once and mirrors it,
    // 3 = it computes the whole square (a measurement switch; "matrix_mirror" = 0 takes the once-per-pair form whatever this says);
    // matrix_smh_path_used = the kernel of the last such call: 1 the fast path (matrix_smh_fast), 0 the generic one, -1 none yet
    int matrix_smh_form = 1;
    int matrix_smh_path_used = -1;

    GraphScratch gs;                    // the graph calls over the result list (host_graph.hpp): their scratch; below, what the last call of each kind reports
    int clusters_last = -1;             // selhip_ctx_cluster: the C of the last call ("clusters_last"), -1 = none yet
    int greedy_clusters_last = -1;      // selhip_ctx_cluster_greedy: the C of the last call ("greedy_clusters_last"), -1 = none yet
    int greedy_rounds_last = -1;        // its rounds ("greedy_rounds_last")
    int forest_rounds_last = -1;        // selhip_ctx_spanning_forest: the rounds of the last call, the empty one included ("forest_rounds_last"), -1 = none yet
    int forest_edges_last = -1;         // its F ("forest_edges_last")
    int linkage_rounds_last = -1;       // selhip_ctx_linkage: the rounds of the last call, rescan rounds and the empty last one included ("linkage_rounds_last"), -1 = none yet
    int linkage_merges_last = -1;       // its F ("linkage_merges_last")
    int linkage_rowscans_last = -1;     // the rows its scan kernel took over all rounds ("linkage_rowscans_last")
    int linkage_rescans_last = -1;      // its rescan rounds ("linkage_rescans_last")

    // sketches merged by group (selhip_ctx_merge_groups; kernel_merge.cuh, host_merge.hpp): scratch the call owns
    MergeScratch mg;
    DevBuf<uint8_t> mg_hll;             // the merged main registers where the caller takes the cardinalities without them

    int timing = 0;                     // 0 off, 1 every kernel scope, 2 dominant stage-1 kernel only
    int dominant_timer = T_STAGE1;
    int timed_kernel = 0;               // timing level 2 keeps the events of: 0 = the stage-1 kernel (join / stream), 1 = stage 2a ("timed_kernel")
    long timed_passes = 0;              // passes under timing: the divisor of every pass timer
    long timed_calls[T_COUNT] = {};     // per call timer (TimedCall), its calls under timing: the divisor of that timer alone (the passes' per-pass averages are not theirs to dilute)
    int last_attempts = 0;              // enqueues the last finished run needed (1 = nothing overflowed)
    KernelTimer timers[T_COUNT];
};

namespace {

// a call timed per call under a name of its own (T_MATRIX and the ids behind it): its timer is the dominant one while it runs (level 2 keeps its events), its calls are counted apart from the passes
struct TimedCall {
    selhip_ctx* c; int before;
    TimedCall(selhip_ctx* c_, int id, bool count = true) : c(c_), before(c_->dominant_timer) { c->dominant_timer = id; if (c->timing && count) c->timed_calls[id] += 1; }
    ~TimedCall() { c->dominant_timer = before; }
};

int check_device(std::string* err) {
    int cnt = 0;
    hipError_t e = hipGetDeviceCount(&cnt);
    if (e != hipSuccess || cnt <= 0) {
        set_err(err, "no HIP device available (%s)", e == hipSuccess ? "count = 0" : hipGetErrorString(e));
        return SELHIP_E_NODEVICE;
    }
    return SELHIP_OK;
}

// timing level 1: every scope; level 2: only the dominant kernel of the pass (an event pair costs ~5 us of stream time, and a pass of
// the default workload is 0.24 ms).  Handing the pair to the launch itself (hipExtLaunchKernelGGL: the dispatch's own start / end
// timestamps) was built and measured in round 3: same step (0.2427 / 0.2404 against 0.2399 / 0.2414 ms), same kernel figure
// (103.9 against 103.3 us) -- the runtime brackets the dispatch with the same packets either way (gpurun_out/r03/t_*).  Not kept.
struct TimerScope {
    selhip_ctx* c; int id; hipStream_t st; hipEvent_t a = nullptr, b = nullptr; bool on;
    TimerScope(selhip_ctx* c_, int id_) : TimerScope(c_, id_, c_->stream) {}
    TimerScope(selhip_ctx* c_, int id_, hipStream_t st_) : c(c_), id(id_), st(st_) {
        on = c->timing == 1 || (c->timing == 2 && id == c->dominant_timer);
        if (on) {
            (void)hipEventCreate(&a); (void)hipEventCreate(&b);
            (void)hipEventRecord(a, st);
        }
    }
    ~TimerScope() {
        if (on) {
            (void)hipEventRecord(b, st);
            c->timers[id].ev.emplace_back(a, b);
            c->timers[id].ev_pass.push_back(c->timed_passes);
        }
    }
};

// where one stage-1 launch (a chunk of query rows) writes: its stream, its slice of the candidate / survivor lists
// and its own counter block; pc0 (the pass's block 0) carries what every chunk reads (z0) and the result counter
struct StageIO {
    hipStream_t st;
    selhip_int2_t* cand;
    selhip_int2_t* surv;
    u64 cap;
    PassCounters* pc;
    int* row_cnt = nullptr;     // if set, the producer of `surv` also tallies survivors per query row (stage-2 grouping)
    int* row_lab = nullptr;     // ... and every row's smallest partner (label order of the grouping)
    u64* seg_cnt = nullptr;     // 16-bit join: this launch's kAppendSegs append counters
};

void drain_timers(selhip_ctx* c) {
    for (int t = 0; t < T_COUNT; ++t) {
        KernelTimer& kt = c->timers[t];
        for (size_t j = 0; j < kt.ev.size();) {
            // the launches of one pass: sum of their durations, and the span they cover together
            size_t e = j;
            float lo = 0, hi = 0;
            for (; e < kt.ev.size() && kt.ev_pass[e] == kt.ev_pass[j]; ++e) {
                float ms = 0, a_off = 0, b_off = 0;
                if (hipEventSynchronize(kt.ev[e].second) != hipSuccess) continue;
                if (hipEventElapsedTime(&ms, kt.ev[e].first, kt.ev[e].second) == hipSuccess) { kt.total_ms += ms; kt.launches += 1; }
                if (hipEventElapsedTime(&a_off, kt.ev[j].first, kt.ev[e].first) == hipSuccess &&
                    hipEventElapsedTime(&b_off, kt.ev[j].first, kt.ev[e].second) == hipSuccess) { lo = std::min(lo, a_off); hi = std::max(hi, b_off); }
            }
            kt.span_ms += hi - lo;
            j = e;
        }
        for (auto& pr : kt.ev) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
        kt.ev.clear(); kt.ev_pass.clear();
    }
}

// stage 2 works on a list bucketed by query row (and laid out by label) unless the caller switched that off -- or the set is small:
// up to group_min_n genomes (2 048) the whole table of bit planes (<= 20 MB) stays in L2 / the Infinity Cache whatever the order, and
// the two grouping launches are 13 us of a 95 us step (BASELINE configs[1])
bool grouping_on(const selhip_ctx* c) { return c->p == 14 && c->group_stage2 && c->n > c->group_min_n; }

// RowMap of the query rows [rb, re) under the context's interleave setting (selhip_ctx_set_row_interleave)
RowMap row_map(const selhip_ctx* c, int rb, int re) {
    RowMap rm;
    rm.row_begin = rb; rm.row_end = re;
    if (c->il_parts > 1) { rm.block_rows = c->il_block; rm.n_parts = c->il_parts; rm.part = c->il_part; }
    else                 { rm.block_rows = std::max(1, re - rb); rm.n_parts = 1; rm.part = 0; }
    return rm;
}

}  // namespace

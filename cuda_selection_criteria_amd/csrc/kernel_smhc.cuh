// kernel_smhc.cuh -- stage 1 of criterion smh_c (SELHIP_CRIT_SMH_C): a pair of the pass's pair space survives iff
//     c(i, k) = #{ j < m : aux_i[j] == aux_k[j] }  >=  c_min            (the full 64 bits of a bucket are compared)
// i.e. the SuperMinHash Jaccard estimate c / m is at least c_min / m.  The count is the cell of kernel_matrix_smh.cuh; here it never leaves
// the scalar unit: no lane write, no dense store, one scalar compare per pair and an append for the few pairs that pass.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).  All kernels read `aux`
// row-major, as uploaded or attached: for a count any lane <-> bucket map does, as long as both rows of a pair use the same one
// (DESIGN.md section 14), so there is no interleaved copy as in ALGO_STREAM.
//   smh_count_kernel<NCH, QUERY, RULE, EMIT, TOPK>  m = 128 * NCH buckets, NCH in {1, 2, 4, 8} (smhc_fast): smh_stream_kernel's block shape and enumeration
//   smh_count_narrow_kernel<G, QUERY, RULE, EMIT, TOPK> m = 128 / G buckets, G in {2, 4}: the same block and enumeration, a wave load = G consecutive
//                                                    candidate rows, the G counts split from two ballots on the scalar unit
//   smh_count_wide_kernel<QUERY, RULE, EMIT, TOPK>  m = 1024 C buckets, C = 2 .. 8: the same block, the chunk walked in spans of 64 candidates, the
//                                                    buckets in C chunks of 1 024 with a running total per (row, lane = candidate) (section 37)
//   smh_count_generic_kernel<QUERY, RULE, EMIT, TOPK> every other m > 0: smh_generic_kernel's unit, lane = candidate, a serial loop over the buckets;
//                                                    also every m under "smhc_generic"
// (smhc_kind(m) says which; the narrow and the wide kernel count with matrix_smh_narrow_counts / matrix_smh_chunk_count of kernel_matrix_smh.cuh)
// QUERY = false: the all-pairs pass (rows and candidates from one set, the window of row i is [max(i + 1, z0), hi[i]], records (i, k));
// QUERY = true: the query pass (rows from Q, candidates from D, the window of query i is [lo[i], hi[i]] of query_windows_kernel, records
// (i, n_q + k) in the combined index space of stage 2).  The pair-list form is pairs_count_kernel (kernel_pairs.cuh).
// Every kernel decides with smhc_selects: THE threshold step, written once.
// RULE (a template argument of all three count kernels): kSmhcFixed -- the threshold is c_min for every pair, the kernels as they were
// before the rule existed, instruction for instruction; kSmhcContainment -- the threshold of pair (i, k) is
//     max(c_min, selhip::smhc_threshold(m, gamma, min(e_i, e_k), max(e_i, e_k)))          (pair_value.hpp; c_min = 0 when never set)
// the count a minimum containment gamma asks for (selhip_ctx_set_min_containment).
// EMIT (the last template argument of all three, false = the kernels as they were before it existed, instruction for instruction): the
// pass's estimator is SELHIP_ESTIMATOR_SMH (selhip_ctx_set_estimator).  A pair that passes the count test is
// COUNTED in n_survivors -- nothing is stored for it -- and, at the point where its count is still at hand, takes
//     V = selhip::smh_value(measure, m, c, e_i, e_k) >= tau                                (pair_value.hpp)
// and goes as the 16-byte record {i, k, V} into the RESULT list behind n_results: the pass has no stage 2.  Query records carry the
// database rank k itself (the index space query_result_fixup_kernel restores for the other criteria).
// TOPK (the last template argument of all four count kernels, false = the kernels as they were before it existed, instruction for
// instruction; QUERY = false, EMIT = true only): one round of an all-pairs top-k pass in row rounds (selhip_ctx_set_topk_rounds, DESIGN.md
// section 19).  A pair with V >= tau is COUNTED in n_final -- the |S| of the one-shot pass -- and its record is appended only if it is
// ADMITTED: V >= thr[i] || V >= thr[k], thr[g] the value of genome g's K-th best record so far (-inf while it holds fewer than K).
// Where the thresholds live: the tile and the generic kernel read both behind the branch; the narrow kernel keeps thr[i] of its tile rows
// in SGPR pairs from block start and reads thr[k] behind the branch; the wide kernel, whose lanes are candidates, keeps thr[i] of a
// wave's rows in SGPR pairs and fetches thr[k] per lane, one coalesced load a span.
#pragma once

// v_writelane_b32 for the wide kernel's running totals: kernel_matrix_smh.cuh's declaration, word for word (that header comes later in
// the translation unit, behind host_plan.hpp, and says why the intrinsic is spelled this way; repeating a declaration or an identical
// macro is well-formed)
#if defined(__has_builtin) && __has_builtin(__builtin_amdgcn_writelane)
#define matrix_smh_writelane(value, lane_idx, old) __builtin_amdgcn_writelane((value), (lane_idx), (old))
#else
__device__ int matrix_smh_writelane(int value, int lane_idx, int old) __asm("llvm.amdgcn.writelane.i32");
#endif

namespace {

// the two counting functions of kernel_matrix_smh.cuh that the narrow and the wide kernel below reuse (defined there, later in the
// translation unit)
template <int G> __device__ __forceinline__ void matrix_smh_narrow_counts(const u64x2& q, const u64x2& cand, int (&cnt)[G]);
template <int NCH> __device__ __forceinline__ int matrix_smh_chunk_count(const u64x2 (&q)[NCH], const u64x2 (&cand)[NCH]);

constexpr bool smhc_fast(int m) { return m == 128 || m == 256 || m == 512 || m == 1024; }
// which kernel a count pass over rows of m buckets takes ("smhc_kernel_used"): the tile kernel where smhc_fast; rows of less than one wave
// load, m = 32 and 64, the narrow kernel; every multiple of 1024 from 2048 to 8192 the wide one; every other m the generic one
enum { kSmhcGeneric = 0, kSmhcTile = 1, kSmhcNarrow = 2, kSmhcWide = 3 };
constexpr int smhc_kind(int m) {
    return smhc_fast(m) ? kSmhcTile : m == 32 || m == 64 ? kSmhcNarrow : m >= 2048 && m <= 8192 && m % 1024 == 0 ? kSmhcWide : kSmhcGeneric;
}
// query rows a wave of the fast path keeps in VGPRs: the stream kernel's budget, at most 12 rows (24 rows at m = 128 unrolled into more
// lane masks in flight than the wave has SGPRs: 25 spilled in the all-pairs form, 6 in the query form -- the matrix kernel's finding)
// (tight = the emit form under the containment rule: its threshold, measure, tally and second counter on top of the rule's one SGPR per
//  row spilled 12 SGPRs in the all-pairs form and 4 in the query form at m = 128 and 256 with 12 rows: 8 rows there)
// (tight = 2, the round form -- TOPK -- of that: the threshold array and the tally of |S| on top spilled 2 SGPRs with 8 rows there: 6 rows;
//  the round form under the fixed rule takes the 8 rows of tight = 1: 90 SGPRs, nothing spilled)
constexpr int smhc_q(int nch, int tight = 0) {
    const int q = kQueryVgprBudget / nch < 12 ? kQueryVgprBudget / nch : 12;
    const int cap = tight == 2 ? 6 : 8;
    return tight && nch <= 2 && q > cap ? cap : q;
}
// the `tight` of a form
constexpr int smhc_tight(bool emit, bool containment, bool topk) { return !emit ? 0 : topk ? (containment ? 2 : 1) : containment ? 1 : 0; }

// the threshold step of every smh_c kernel
__device__ __forceinline__ bool smhc_selects(int count, int c_min) { return count >= c_min; }

constexpr int kSmhcFixed = 0, kSmhcContainment = 1;
// what the containment rule reads besides the counts: gamma and the truncated cardinalities of the rows (ex) and the candidates (ey);
// the same array in the all-pairs pass and in a pair list
struct SmhcRule { double gamma; const u64* __restrict__ ex; const u64* __restrict__ ey; };
// what the emit form reads besides: the threshold and the measure of V, and the pass's counter block 0 (n_results).  It rides behind
// the rule in the kernels' last argument, so the form that emits nothing keeps its argument list to the byte
struct SmhcEmit { double tau; int measure; PassCounters* __restrict__ pc0; };
struct SmhcRuleEmit : SmhcRule { SmhcEmit em; };
// what a round of a top-k pass in row rounds reads besides: every genome's admission threshold as it stood when the round began.  It
// rides behind the emit operands in the same way
struct SmhcRuleEmitTopk : SmhcRuleEmit { const double* __restrict__ thr; };
template <bool EMIT, bool TOPK = false> using SmhcRuleArg = std::conditional_t<TOPK, SmhcRuleEmitTopk, std::conditional_t<EMIT, SmhcRuleEmit, SmhcRule>>;
template <bool EMIT> using SmhcRecord = std::conditional_t<EMIT, selhip_pair_t, selhip_int2_t>;
// the record of a pair under the estimator, or nothing: *sel = V >= tau (false for NaN)
__device__ __forceinline__ selhip_pair_t smhc_record(const SmhcEmit& em, int m, int cnt, u64 e1, u64 e2, int i, int k, bool* sel) {
    selhip_pair_t r;
    r.i = i; r.k = k; r.jaccard = selhip::smh_value(em.measure, m, cnt, e1, e2);
    *sel = r.jaccard >= em.tau;
    return r;
}
// the wave's tally of pairs that passed the count test: one atomic without a return value, and none for a wave without such a pair
__device__ __forceinline__ void smhc_tally(u64* __restrict__ n_survivors, int n_pass, int lane) {
    if (n_pass != 0 && lane == 0) atomicAdd(n_survivors, (u64)n_pass);
}
// THE admission test of a round, written once: non-strict, so that a tie with an owner's K-th value reaches the select, where the
// partner rank decides.  Two uniform f64 loads and two compares, behind the pinned branch
__device__ __forceinline__ bool smhc_admits(const double* __restrict__ thr, int i, int k, double v) { return v >= thr[i] || v >= thr[k]; }
// the same test for a kernel that holds the two thresholds in registers already (narrow: thr[i] in an SGPR pair; wide: thr[k] per lane):
// smhc_admits on a local pair, which the compiler dissolves into the two compares
__device__ __forceinline__ bool smhc_admits_held(double thr_i, double thr_k, double v) {
    const double held[2] = {thr_i, thr_k};
    return smhc_admits(held, 0, 1, v);
}
// the exact threshold of a pair under the containment rule
__device__ __forceinline__ int smhc_pair_threshold(int m, double gamma, u64 e1, u64 e2, int c_min) {
    return max(c_min, selhip::smhc_threshold(m, gamma, e1 < e2 ? e1 : e2, e1 < e2 ? e2 : e1));
}

// the count of the fast path: 2 NCH v_cmp_eq_u64 lane masks, one s_bcnt1_i32_b64 each, scalar adds (wave-uniform result)
template <int NCH>
__device__ __forceinline__ int smhc_count(const u64x2 (&cand)[NCH], const u64x2 (&q)[NCH]) {
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c)
        cnt += __popcll(__ballot(cand[c].x == q[c].x)) + __popcll(__ballot(cand[c].y == q[c].y));
    return cnt;
}

// the count of the lane-serial kernels: one lane walks both rows
__device__ __forceinline__ int smhc_count_lane(const u64* __restrict__ x, const u64* __restrict__ y, int m) {
    int cnt = 0;
    for (int b = 0; b < m; ++b) cnt += x[b] == y[b] ? 1 : 0;
    return cnt;
}

// the pair space of both kernels: the window of row i, and the record of (i, k)
template <bool QUERY>
struct SmhcSpace {
    const int* __restrict__ lo;     // QUERY: first candidate of every query's window; else unused
    const int* __restrict__ hi;     // last candidate of every row's window
    int z0;                         // !QUERY: first candidate rank of the pass (first rank with e != 0, raised to cand_begin)
    int n_x;                        // rows of X (QUERY: n_q, the offset of D in the combined index space)
    __device__ __forceinline__ int first(int i) const { return QUERY ? lo[i] : max(i + 1, z0); }
    __device__ __forceinline__ bool holds(int i, int k) const { return k >= first(i) && k <= hi[i]; }
    __device__ __forceinline__ int partner(int k) const { return QUERY ? n_x + k : k; }
};

// ---------------------------------------------------------------------------------------------
// smh_count_kernel<NCH, QUERY, RULE>
//   block  = 4 waves; one block = (tile of Q = smhc_q(NCH) rows of X) x (chunk of kChunk candidates of Y), blockIdx.x -> (tile =
//            b % n_tiles, chunk = b / n_tiles) as in smh_stream_kernel: the blocks of a chunk share it through their XCD's L2
//   rows   = every wave holds the tile's Q rows in VGPRs, loaded coalesced (load c of a row hands lane l the buckets 128 c + 2 l, + 1)
//   stream = the wave walks its candidates (stride 4), NCH x global_load_dwordx4 per candidate, kStreamAhead candidates ahead in a ring
//            of register sets addressed statically
//   pair   = smhc_count, ONE scalar compare against c_min, app.push_uniform for a pair that passes and lies in the row's window
// RULE = kSmhcContainment: the scalar compare of a pair goes against its ROW's coarse threshold, one SGPR per tile row computed at block
// start: a lower bound of the exact threshold over the block's candidates [max(k0, kmin), k_end), raised to c_min.  The threshold is
// non-increasing in the larger cardinality and the ranks ascend in cardinality, so in the all-pairs pass (k > i: e_k >= e_i) the bound
// is the threshold at the range's last candidate; in a query pass the threshold rises while e_k < e_i and falls from there on, so its
// minimum over the range is at one of the two ends.  (A range end with e = 0 -- threshold m + 1 by definition, outside that shape --
// gives the bound 0.)  A chunk is kChunk consecutive ranks of a sorted set: the bound is tight.  Only a pair that passes it takes the
// exact test -- one f64 divide on uniform operands -- behind the pinned branch, beside the window test.
// The count is never cut short (no "count + remaining buckets < c_min" exit): the test would be a scalar compare and branch per
// ballot on the path every pair takes, where the whole count costs one s_bcnt1 and one s_add per ballot.
// No LDS tile and no block barrier: a wave that has no candidate leaves on its own.
// ---------------------------------------------------------------------------------------------
template <int NCH, bool QUERY, int RULE, bool EMIT = false, bool TOPK = false>
__global__ __launch_bounds__(kBlock, (NCH <= 4 ? 3 : 2))
void smh_count_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_x, int n_y,
                      const int* __restrict__ lo, const int* __restrict__ hi, const PassCounters* __restrict__ pc_in,
                      RowMap rm, int n_tiles, int chunk_base, int c_min,
                      SmhcRecord<EMIT>* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, SmhcRuleArg<EMIT, TOPK> rule) {
    static_assert(!TOPK || (EMIT && !QUERY), "the round form is an all-pairs pass that emits");
    constexpr int Q = smhc_q(NCH, smhc_tight(EMIT, RULE == kSmhcContainment, TOPK));
    constexpr int ROWV = NCH * kWave;                 // u64x2 per sketch row
    __shared__ SmhcRecord<EMIT> app_lds[kWavesPerBlock * kAppendCap];

    const int tile = blockIdx.x % n_tiles;
    const int chunk = blockIdx.x / n_tiles;
    int i0, i_end;
    rm.tile_rows(tile, Q, &i0, &i_end);
    if (i0 >= i_end) return;
    const int i_last = i_end - 1;
    SmhcSpace<QUERY> sp{lo, hi, 0, n_x};
    int kmin, kmax;
    if constexpr (QUERY) {
        kmin = 0x7FFFFFFF; kmax = -1;
        for (int i = i0; i < i_end; ++i) {            // uniform loads; an empty window (hi < lo) takes no part
            const int l = lo[i], h = hi[i];
            if (h >= l) { kmin = min(kmin, l); kmax = max(kmax, h); }
        }
    } else {
        sp.z0 = pc_in->z0p1 ? pc_in->z0p1 - 1 : n_y;
        kmin = max(i0 + 1, sp.z0);
        kmax = hi[i_last];                            // hi is non-decreasing in i
    }
    const int k0 = chunk_base + chunk * kChunk;
    if (k0 > kmax || k0 + kChunk - 1 < kmin) return;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);     // wave-uniform -> SGPR loop counter
    const int k_end = min(min(k0 + kChunk, n_y), kmax + 1);
    int k = max(k0, kmin) + wave;
    if (k >= k_end) return;

    int coarse[Q];                                                            // RULE = kSmhcContainment: wave-uniform, one SGPR per tile row
    if constexpr (RULE == kSmhcContainment) {
        const int ks = max(k0, kmin);                                        // ks <= k_end - 1 < n_y
        const u64 e_first = rule.ey[ks], e_last = rule.ey[k_end - 1];
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const u64 e_i = rule.ex[min(i0 + a, n_x - 1)];
            int t = selhip::smhc_threshold(128 * NCH, rule.gamma, min(e_i, e_last), max(e_i, e_last));
            if constexpr (QUERY) {
                t = min(t, selhip::smhc_threshold(128 * NCH, rule.gamma, min(e_i, e_first), max(e_i, e_first)));
                if (e_first == 0 || e_i == 0) t = 0;
            }
            coarse[a] = __builtin_amdgcn_readfirstlane(max(t, c_min));
        }
    }

    u64x2 q[Q][NCH];
#pragma unroll
    for (int a = 0; a < Q; ++a) {
        const u64x2* row = X + (long long)min(i0 + a, n_x - 1) * ROWV + lane;        // rows past the end: a valid row, never a record
#pragma unroll
        for (int c = 0; c < NCH; ++c) q[a][c] = row[c * kWave];
    }

    WaveAppenderT<SmhcRecord<EMIT>> app;
    if constexpr (EMIT) app.init(app_lds, wave, surv, surv_cap, &rule.em.pc0->n_results);
    else app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
    int n_pass = 0;                                                           // EMIT: pairs that passed the count test (wave-uniform)
    int n_sel = 0;                                                            // TOPK: those of them with V >= tau (wave-uniform)
    constexpr int AHEAD = NCH <= 4 ? kStreamAhead : 1;                         // (m = 1024: the registers allow one row ahead)
    constexpr int RING = AHEAD + 1;
    u64x2 ring[RING][NCH];
    auto load_row = [&](u64x2 (&dst)[NCH], int kk) {
        const int kc = min(kk, k_end - 1);                                    // clamped: prefetches past the end re-read a valid row
        const u64x2* row = Y + (long long)kc * ROWV + lane;
#pragma unroll
        for (int c = 0; c < NCH; ++c) dst[c] = row[c * kWave];
    };
    auto compare_row = [&](const u64x2 (&cand)[NCH], int kk) {
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const int cnt = smhc_count<NCH>(cand, q[a]);
            if (smhc_selects(cnt, RULE == kSmhcContainment ? coarse[a] : c_min)) {
                // (the empty volatile asm pins the branch on the count alone, as in smh_stream_kernel: the window tests stay off the
                //  path of the pairs that fail it)
                asm volatile("");
                const int i = i0 + a;
                if (i < i_end && sp.holds(i, kk)) {
                    bool ok = true;
                    if constexpr (RULE == kSmhcContainment)
                        ok = smhc_selects(cnt, smhc_pair_threshold(128 * NCH, rule.gamma, rule.ex[i], rule.ey[kk], c_min));
                    if constexpr (EMIT) {
                        if (ok) {
                            n_pass += 1;
                            bool sel;
                            const selhip_pair_t r = smhc_record(rule.em, 128 * NCH, cnt, rule.ex[i], rule.ey[kk], i, kk, &sel);
                            if constexpr (TOPK) {
                                if (sel) {
                                    n_sel += 1;
                                    if (smhc_admits(rule.thr, i, kk, r.jaccard)) app.push_uniform_record(r, lane);
                                }
                            } else {
                                if (sel) app.push_uniform_record(r, lane);
                            }
                        }
                    } else {
                        if (ok) app.push_uniform(i, sp.partner(kk), lane);
                    }
                }
            }
        }
    };
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) load_row(ring[s], k + s * kWavesPerBlock);
    for (; k < k_end; k += RING * kWavesPerBlock) {
#pragma unroll
        for (int s = 0; s < RING; ++s) {
            const int kk = k + s * kWavesPerBlock;
            if (kk >= k_end) break;
            load_row(ring[(s + AHEAD) % RING], kk + AHEAD * kWavesPerBlock);
            compare_row(ring[s], kk);
        }
    }
    app.flush(lane);
    if constexpr (EMIT) smhc_tally(&pc->n_survivors, n_pass, lane);
    if constexpr (TOPK) smhc_tally(&pc->n_final, n_sel, lane);
}

// generic stage 1: block = 256 lanes = 256 candidates of one row; grid = (chunks, rows)
template <bool QUERY, int RULE, bool EMIT = false, bool TOPK = false>
__global__ __launch_bounds__(kBlock)
void smh_count_generic_kernel(const u64* __restrict__ X, const u64* __restrict__ Y, int n_x, int n_y, int m,
                              const int* __restrict__ lo, const int* __restrict__ hi, const PassCounters* __restrict__ pc_in,
                              RowMap rm, int n_rows_grid, int c_min,
                              SmhcRecord<EMIT>* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, SmhcRuleArg<EMIT, TOPK> rule) {
    static_assert(!TOPK || (EMIT && !QUERY), "the round form is an all-pairs pass that emits");
    __shared__ SmhcRecord<EMIT> app_lds[kWavesPerBlock * kAppendCap];
    int i, i_e;
    rm.tile_rows((int)(blockIdx.x % n_rows_grid), 1, &i, &i_e);
    const int chunk = blockIdx.x / n_rows_grid;
    if (i >= i_e) return;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    SmhcSpace<QUERY> sp{lo, hi, 0, n_x};
    if constexpr (!QUERY) sp.z0 = pc_in->z0p1 ? pc_in->z0p1 - 1 : n_y;
    const int kmax = hi[i];
    const long long kl = (long long)sp.first(i) + (long long)chunk * kBlock + (int)threadIdx.x;
    const bool in_range = kl <= kmax && kl < n_y;
    const int k = in_range ? (int)kl : 0;
    int t = c_min;
    if constexpr (RULE == kSmhcContainment) t = smhc_pair_threshold(m, rule.gamma, rule.ex[i], rule.ey[k], c_min);      // (k = 0 out of range: a valid rank)
    if constexpr (EMIT) {
        const int cnt = in_range ? smhc_count_lane(X + (long long)i * m, Y + (long long)k * m, m) : 0;
        const bool ok = in_range && smhc_selects(cnt, t);
        WaveRecordAppender app;
        app.init(app_lds, wave, surv, surv_cap, &rule.em.pc0->n_results);
        bool sel;
        const selhip_pair_t r = smhc_record(rule.em, m, cnt, rule.ex[i], rule.ey[k], i, k, &sel);       // (k = 0 out of range: a valid rank)
        if constexpr (TOPK) app.push_record(ok && sel && smhc_admits(rule.thr, i, k, r.jaccard), r, lane);      // (k = 0 out of range: a valid rank)
        else app.push_record(ok && sel, r, lane);
        app.flush(lane);
        smhc_tally(&pc->n_survivors, (int)__popcll(__ballot(ok)), lane);
        if constexpr (TOPK) smhc_tally(&pc->n_final, (int)__popcll(__ballot(ok && sel)), lane);
    } else {
        const bool ok = in_range && smhc_selects(smhc_count_lane(X + (long long)i * m, Y + (long long)k * m, m), t);
        WaveAppender app;
        app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
        app.push(ok, i, sp.partner(k), lane);
        app.flush(lane);
    }
}

// ---------------------------------------------------------------------------------------------
// smh_count_narrow_kernel<G, QUERY, RULE, EMIT>      m = 128 / G buckets, G in {2, 4}: a row is 1 / G of a wave load
//   block  = smh_count_kernel's: (tile of Q = smhc_narrow_q(EMIT, RULE) rows of X) x (chunk of kChunk candidates of Y), the same RowMap, windows, early
//            exits and appender
//   rows   = ONE u64x2 per row: lane l holds buckets 2 (l % (64 / G)), + 1, so each of the G lane groups holds the whole row
//   stream = a wave load is G CONSECUTIVE candidates kk .. kk + G - 1, lane group g holding row kk + g (matrix_smh_narrow_kernel's packing);
//            wave w starts at max(k0, kmin) + w G and strides 4 G, kStreamAhead loads ahead in the ring
//   pair   = matrix_smh_narrow_counts<G> splits the two ballots into the G counts on the scalar unit; each count takes ONE scalar compare
//            (c_min, or the row's coarse threshold) and only one that passes goes behind the pinned branch
// The two edges.  (1) The last load of a walk may reach past k_end: its lane groups past the end re-read row k_end - 1 (a per-lane min),
// and `kk + g < k_end` behind the branch keeps their counts from ever becoming a record or a tally -- the same test keeps a load that
// straddles the chunk's end from counting the next chunk's candidates twice (max(k0, kmin) is on no grid of G).  (2) A load may begin
// before first(i): sp.holds decides per (i, kk + g), as in the tile kernel.
// Q: 12 rows (48 VGPRs) under the fixed rule, emitting or not.  Under the containment rule the row's coarse threshold takes an SGPR per
// row on top of the G counts in flight, and 12 rows spilled SGPRs (to VGPR lanes, no scratch): 1 (m = 64) and 2 (m = 32) in the all-pairs
// form, 14 and 15 in its emit form, 6 in the query pass's emit form -- so, as smhc_q's `tight` does, 10 rows there and 8 where the pass
// emits as well (resource lines: DESIGN.md section 37).
// The round form (TOPK) keeps thr[i] of every tile row in an SGPR pair on top of that, so that the admission test behind the branch reads
// thr[k] alone.  With the emit form's rows it spilled 23 SGPRs under the fixed rule (12 rows; 9 / 10 with 10 rows, 3 / 5 with 9) and 13 / 15
// under the containment rule (8 rows; 0 / 2 with 6): 8 rows and 5 rows there, nothing spilled.
// ---------------------------------------------------------------------------------------------
constexpr int smhc_narrow_q(bool emit, bool containment, bool topk = false) { return topk ? (containment ? 5 : 8) : !containment ? 12 : emit ? 8 : 10; }
template <int G, bool QUERY, int RULE, bool EMIT = false, bool TOPK = false>
__global__ __launch_bounds__(kBlock, 3)
void smh_count_narrow_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_x, int n_y,
                             const int* __restrict__ lo, const int* __restrict__ hi, const PassCounters* __restrict__ pc_in,
                             RowMap rm, int n_tiles, int chunk_base, int c_min,
                             SmhcRecord<EMIT>* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, SmhcRuleArg<EMIT, TOPK> rule) {
    static_assert(!TOPK || (EMIT && !QUERY), "the round form is an all-pairs pass that emits");
    constexpr int Q = smhc_narrow_q(EMIT, RULE == kSmhcContainment, TOPK);
    constexpr int LPR = kWave / G;                    // u64x2 (lanes) per sketch row: m = 2 LPR
    constexpr int M = 2 * LPR;
    __shared__ SmhcRecord<EMIT> app_lds[kWavesPerBlock * kAppendCap];

    const int tile = blockIdx.x % n_tiles;
    const int chunk = blockIdx.x / n_tiles;
    int i0, i_end;
    rm.tile_rows(tile, Q, &i0, &i_end);
    if (i0 >= i_end) return;
    const int i_last = i_end - 1;
    SmhcSpace<QUERY> sp{lo, hi, 0, n_x};
    int kmin, kmax;
    if constexpr (QUERY) {
        kmin = 0x7FFFFFFF; kmax = -1;
        for (int i = i0; i < i_end; ++i) {            // uniform loads; an empty window (hi < lo) takes no part
            const int l = lo[i], h = hi[i];
            if (h >= l) { kmin = min(kmin, l); kmax = max(kmax, h); }
        }
    } else {
        sp.z0 = pc_in->z0p1 ? pc_in->z0p1 - 1 : n_y;
        kmin = max(i0 + 1, sp.z0);
        kmax = hi[i_last];                            // hi is non-decreasing in i
    }
    const int k0 = chunk_base + chunk * kChunk;
    if (k0 > kmax || k0 + kChunk - 1 < kmin) return;

    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    const int sub = lane & (LPR - 1), grp = lane / LPR;                       // this lane's place in its row, its row in the load
    const int k_end = min(min(k0 + kChunk, n_y), kmax + 1);
    const int ks = max(k0, kmin);
    int k = ks + wave * G;
    if (k >= k_end) return;

    int coarse[Q];                                                            // RULE = kSmhcContainment: smh_count_kernel's bound, one SGPR per tile row
    if constexpr (RULE == kSmhcContainment) {
        const u64 e_first = rule.ey[ks], e_last = rule.ey[k_end - 1];        // ks <= k_end - 1 < n_y
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const u64 e_i = rule.ex[min(i0 + a, n_x - 1)];
            int t = selhip::smhc_threshold(M, rule.gamma, min(e_i, e_last), max(e_i, e_last));
            if constexpr (QUERY) {
                t = min(t, selhip::smhc_threshold(M, rule.gamma, min(e_i, e_first), max(e_i, e_first)));
                if (e_first == 0 || e_i == 0) t = 0;
            }
            coarse[a] = __builtin_amdgcn_readfirstlane(max(t, c_min));
        }
    }

    double thr_i[Q];                                                          // TOPK: the tile rows' thresholds, wave-uniform, one SGPR pair per row
    if constexpr (TOPK) {
#pragma unroll
        for (int a = 0; a < Q; ++a) thr_i[a] = rule.thr[min(i0 + a, n_x - 1)];                // (uniform address: a scalar load; rows past the end as below)
    }

    u64x2 q[Q];
#pragma unroll
    for (int a = 0; a < Q; ++a) q[a] = X[(long long)min(i0 + a, n_x - 1) * LPR + sub];      // rows past the end: a valid row, never a record

    WaveAppenderT<SmhcRecord<EMIT>> app;
    if constexpr (EMIT) app.init(app_lds, wave, surv, surv_cap, &rule.em.pc0->n_results);
    else app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
    int n_pass = 0;                                                           // EMIT: pairs that passed the count test (wave-uniform)
    int n_sel = 0;                                                            // TOPK: those of them with V >= tau (wave-uniform)
    constexpr int AHEAD = kStreamAhead;
    constexpr int RING = AHEAD + 1;
    constexpr int STEP = kWavesPerBlock * G;                                  // candidates between two loads of a wave
    u64x2 ring[RING];
    // rows kk .. kk + G - 1, one per lane group; a group past the end re-reads row k_end - 1
    auto load_rows = [&](u64x2& dst, int kk) { dst = Y[(long long)min(kk + grp, k_end - 1) * LPR + sub]; };
    auto compare_rows = [&](const u64x2& cand, int kk) {
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            int cnt[G];
            matrix_smh_narrow_counts<G>(q[a], cand, cnt);
#pragma unroll
            for (int g = 0; g < G; ++g) {
                if (smhc_selects(cnt[g], RULE == kSmhcContainment ? coarse[a] : c_min)) {
                    asm volatile("");                                         // (pins the branch on the count alone, as in smh_count_kernel)
                    const int i = i0 + a, kg = kk + g;
                    if (i < i_end && kg < k_end && sp.holds(i, kg)) {
                        bool ok = true;
                        if constexpr (RULE == kSmhcContainment)
                            ok = smhc_selects(cnt[g], smhc_pair_threshold(M, rule.gamma, rule.ex[i], rule.ey[kg], c_min));
                        if constexpr (EMIT) {
                            if (ok) {
                                n_pass += 1;
                                bool sel;
                                const selhip_pair_t r = smhc_record(rule.em, M, cnt[g], rule.ex[i], rule.ey[kg], i, kg, &sel);
                                if constexpr (TOPK) {
                                    if (sel) {
                                        n_sel += 1;
                                        if (smhc_admits_held(thr_i[a], rule.thr[kg], r.jaccard)) app.push_uniform_record(r, lane);
                                    }
                                } else {
                                    if (sel) app.push_uniform_record(r, lane);
                                }
                            }
                        } else {
                            if (ok) app.push_uniform(i, sp.partner(kg), lane);
                        }
                    }
                }
            }
        }
    };
#pragma unroll
    for (int s = 0; s < AHEAD; ++s) load_rows(ring[s], k + s * STEP);
    for (; k < k_end; k += RING * STEP) {
#pragma unroll
        for (int s = 0; s < RING; ++s) {
            const int kk = k + s * STEP;
            if (kk >= k_end) break;
            load_rows(ring[(s + AHEAD) % RING], kk + AHEAD * STEP);
            compare_rows(ring[s], kk);
        }
    }
    app.flush(lane);
    if constexpr (EMIT) smhc_tally(&pc->n_survivors, n_pass, lane);
    if constexpr (TOPK) smhc_tally(&pc->n_final, n_sel, lane);
}

// ---------------------------------------------------------------------------------------------
// smh_count_wide_kernel<QUERY, RULE, EMIT, TOPK>    m = 1024 C buckets, C = 2 .. 8 (a kernel argument): the buckets are split, not the rows
//   block  = (tile of 12 rows of X: 4 waves x Q = 3 rows) x (chunk of kChunk candidates of Y), blockIdx.x -> (tile, chunk) as above.  A
//            wave cuts the chunk to the windows of ITS three rows and walks what is left in spans of 64 candidates
//   span   = matrix_smh_wide_kernel's: per bucket chunk c the wave's 3 query chunks in 96 VGPRs, the span's candidate chunks streamed past
//            them through a ring of two register sets (ONE stream of (chunk, candidate) steps), matrix_smh_chunk_count<8> per step, the
//            count added into lane (candidate - span start) of the row's running total (v_readlane_b32, s_add_i32, v_writelane_b32)
//   tail   = after the last bucket chunk lane = candidate: each lane tests its total against the threshold and, behind it, the window
//            and the exact rule; survivors leave through the per-lane push forms of the generic kernel, the tallies come from ballots
// The four waves of a block hold different rows, so each of them walks every span its rows reach, all in the same order from the same
// start: they stay within a few rows of each other and the span's 64 C x 8 KiB are fetched from L2 once for the four of them (no
// barrier keeps them together; a wave whose rows end early leaves on its own).
// RULE = kSmhcContainment: no coarse bound.  Lanes are candidates here, so the exact threshold of (row, lane) is computed once per span
// and row -- one f64 divide per lane against the 16 C compares per lane and row of the span -- and the compare of the tail is exact.
// ---------------------------------------------------------------------------------------------
constexpr int kSmhcWideNch = 8;                        // wave loads per bucket chunk: 1 024 buckets, the tile kernel's widest row
constexpr int kSmhcWideQ = 3;                          // rows a wave keeps (one bucket chunk each): 96 VGPRs
template <bool QUERY, int RULE, bool EMIT = false, bool TOPK = false>
__global__ __launch_bounds__(kBlock, 2)
void smh_count_wide_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_x, int n_y, int n_bch,
                           const int* __restrict__ lo, const int* __restrict__ hi, const PassCounters* __restrict__ pc_in,
                           RowMap rm, int n_tiles, int chunk_base, int c_min,
                           SmhcRecord<EMIT>* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, SmhcRuleArg<EMIT, TOPK> rule) {
    static_assert(!TOPK || (EMIT && !QUERY), "the round form is an all-pairs pass that emits");
    constexpr int NCH = kSmhcWideNch;
    constexpr int Q = kSmhcWideQ;
    constexpr int CHV = NCH * kWave;                   // u64x2 per bucket chunk of a row
    const long long pitch = (long long)n_bch * CHV;    // u64x2 per sketch row
    const int m = 2 * CHV * n_bch;
    __shared__ SmhcRecord<EMIT> app_lds[kWavesPerBlock * kAppendCap];

    const int tile = blockIdx.x % n_tiles;
    const int chunk = blockIdx.x / n_tiles;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
    int t0, t_end;
    rm.tile_rows(tile, kWavesPerBlock * Q, &t0, &t_end);
    const int i0 = t0 + wave * Q, i_end = min(i0 + Q, t_end);                 // this wave's rows
    if (i0 >= i_end) return;                                                  // (no block barrier below)
    SmhcSpace<QUERY> sp{lo, hi, 0, n_x};
    int kmin, kmax;
    if constexpr (QUERY) {
        kmin = 0x7FFFFFFF; kmax = -1;
        for (int i = i0; i < i_end; ++i) {            // uniform loads; an empty window (hi < lo) takes no part
            const int l = lo[i], h = hi[i];
            if (h >= l) { kmin = min(kmin, l); kmax = max(kmax, h); }
        }
    } else {
        sp.z0 = pc_in->z0p1 ? pc_in->z0p1 - 1 : n_y;
        kmin = max(i0 + 1, sp.z0);
        kmax = hi[i_end - 1];                         // hi is non-decreasing in i
    }
    const int k0 = chunk_base + chunk * kChunk;
    if (k0 > kmax || k0 + kChunk - 1 < kmin) return;
    const int k_end = min(min(k0 + kChunk, n_y), kmax + 1);

    WaveAppenderT<SmhcRecord<EMIT>> app;
    if constexpr (EMIT) app.init(app_lds, wave, surv, surv_cap, &rule.em.pc0->n_results);
    else app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
    int n_pass = 0;                                                           // EMIT: pairs that passed the count test (wave-uniform)
    int n_sel = 0;                                                            // TOPK: those of them with V >= tau (wave-uniform)
    double thr_i[Q];                                                          // TOPK: the wave's rows' thresholds, wave-uniform, one SGPR pair per row
    if constexpr (TOPK) {
#pragma unroll
        for (int a = 0; a < Q; ++a) thr_i[a] = rule.thr[min(i0 + a, n_x - 1)];                // (uniform address: a scalar load)
    }

    for (int s0 = max(k0, kmin); s0 < k_end; s0 += kWave) {                   // the span [s0, se): lane l <-> candidate s0 + l
        const int se = min(s0 + kWave, k_end);
        // TOPK: the candidates' thresholds, lane l <-> thr[s0 + l] (lanes past the span: thr[se - 1], never a record): ONE coalesced f64
        // load, issued in front of the span's first chunk and first read in the tail, n_bch (se - s0) steps later
        double thr_k = 0.0;
        if constexpr (TOPK) thr_k = rule.thr[min(s0 + lane, se - 1)];
        u64x2 q[Q][NCH];
        auto load_queries = [&](int c) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const u64x2* row = X + (long long)min(i0 + a, n_x - 1) * pitch + (long long)c * CHV + lane;    // rows past the end: a valid row, never a record
#pragma unroll
                for (int h = 0; h < NCH; ++h) q[a][h] = row[h * kWave];
            }
        };
        int acc[Q];                                                           // lane l: the running count of candidate s0 + l
#pragma unroll
        for (int a = 0; a < Q; ++a) acc[a] = 0;
        u64x2 ring[2][NCH];
        int pcn = 0, pk = s0;                                                 // the step to fetch next (wave-uniform): s0 <= pk < se <= n_y, pcn < n_bch
        auto prefetch = [&](u64x2 (&dst)[NCH]) {
            const u64x2* row = Y + (long long)pk * pitch + (long long)pcn * CHV + lane;
#pragma unroll
            for (int h = 0; h < NCH; ++h) dst[h] = row[h * kWave];
            if (pk + 1 < se) ++pk;
            else if (pcn + 1 < n_bch) { pk = s0; ++pcn; }                     // (behind the last step: that step again)
        };
        int cc = 0, ck = s0;                                                  // the step to compare next
        auto compare_row = [&](const u64x2 (&cand)[NCH]) {
            const int col = ck - s0;
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const int cnt = matrix_smh_chunk_count<NCH>(q[a], cand) + __builtin_amdgcn_readlane(acc[a], col);
                acc[a] = matrix_smh_writelane(cnt, col, acc[a]);
            }
            if (++ck == se) {
                ck = s0;
                if (++cc < n_bch) load_queries(cc);
            }
        };
        const int steps = n_bch * (se - s0);
        prefetch(ring[0]);
        load_queries(0);
        for (int t = 0; t < steps; t += 2) {
            prefetch(ring[1]);
            compare_row(ring[0]);
            if (t + 1 >= steps) break;
            prefetch(ring[0]);
            compare_row(ring[1]);
        }
        // the tail: lane = candidate
        const int kl = s0 + lane;
        const bool in_span = kl < se;
        const int kc = min(kl, se - 1);                                       // lanes past the span: a valid rank, never a record
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const int i = i0 + a;
            if (i >= i_end) break;
            const int cnt = acc[a];
            bool ok = in_span && smhc_selects(cnt, c_min);
            if (__ballot(ok) == 0) continue;                                  // (the rule's threshold is never below c_min)
            ok = ok && sp.holds(i, kl);
            if constexpr (RULE == kSmhcContainment)
                ok = ok && smhc_selects(cnt, smhc_pair_threshold(m, rule.gamma, rule.ex[i], rule.ey[kc], c_min));
            if constexpr (EMIT) {
                bool sel;
                const selhip_pair_t r = smhc_record(rule.em, m, cnt, rule.ex[i], rule.ey[kc], i, kl, &sel);
                if constexpr (TOPK) {
                    // the vector form of the admission test: thr[i] uniform, thr[k] and V per lane; only selected AND admitted lanes append
                    app.push_record(ok && sel && smhc_admits_held(thr_i[a], thr_k, r.jaccard), r, lane);
                    n_sel += (int)__popcll(__ballot(ok && sel));
                } else {
                    app.push_record(ok && sel, r, lane);
                }
                n_pass += (int)__popcll(__ballot(ok));
            } else {
                app.push(ok, i, sp.partner(kl), lane);
            }
        }
    }
    app.flush(lane);
    if constexpr (EMIT) smhc_tally(&pc->n_survivors, n_pass, lane);
    if constexpr (TOPK) smhc_tally(&pc->n_final, n_sel, lane);
}

}  // namespace

// kernel_smhc.cuh -- stage 1 of criterion smh_c (SELHIP_CRIT_SMH_C): a pair of the pass's pair space survives iff
//     c(i, k) = #{ j < m : aux_i[j] == aux_k[j] }  >=  c_min            (the full 64 bits of a bucket are compared)
// i.e. the SuperMinHash Jaccard estimate c / m is at least c_min / m.  The count is the cell of kernel_matrix_smh.cuh; here it never leaves
// the scalar unit: no lane write, no dense store, one scalar compare per pair and an append for the few pairs that pass.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).  All kernels read `aux`
// row-major, as uploaded or attached: for a count any lane <-> bucket map does, as long as both rows of a pair use the same one
// (DESIGN.md section 14), so there is no interleaved copy as in ALGO_STREAM.
//   smh_count_kernel<NCH, QUERY, RULE, EMIT, TOPK>  m = 128 * NCH buckets, NCH in {1, 2, 4, 8} (smhc_fast): smh_stream_kernel's block shape and enumeration
//   smh_count_generic_kernel<QUERY, RULE, EMIT, TOPK> every other m > 0: smh_generic_kernel's unit, lane = candidate, a serial loop over the buckets
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
// TOPK (the last template argument of the two count kernels, false = the kernels as they were before it existed, instruction for
// instruction; QUERY = false, EMIT = true only): one round of an all-pairs top-k pass in row rounds (selhip_ctx_set_topk_rounds, DESIGN.md
// section 19).  A pair with V >= tau is COUNTED in n_final -- the |S| of the one-shot pass -- and its record is appended only if it is
// ADMITTED: V >= thr[i] || V >= thr[k], thr[g] the value of genome g's K-th best record so far (-inf while it holds fewer than K).
#pragma once

namespace {

constexpr bool smhc_fast(int m) { return m == 128 || m == 256 || m == 512 || m == 1024; }
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

}  // namespace

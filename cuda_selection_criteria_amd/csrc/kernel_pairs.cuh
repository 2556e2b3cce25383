// kernel_pairs.cuh -- stage 1 of the pair-list passes (selhip_ctx_run_pairs, host_pairs.hpp): the pair space is a caller's list of
// entries {x, y}, not a triangle or a rectangle that the pass enumerates itself.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
#pragma once

namespace {

// =============================================================================================
// What the kernels share.  A block takes kPairsBlock consecutive entries per batch:
//  * every thread reads ONE entry with an 8-byte load (a wave reads 512 contiguous bytes), puts the smaller rank first and decides
//        valid = 0 <= x, y < n and x != y            live = valid && e_hi != 0 && (!use_cb || CB(tau, e_lo, e_hi))
//    from the truncated cards the pass's first kernel wrote (`live` is the entry's membership of the all-pairs pair space E);
//  * the live and the invalid entries are tallied per wave in registers and leave the block as ONE atomic each when the block ends
//    (the pass's block 0: n_evaluated; n_pre = invalid entries, n_pre_segmax = 1 + the largest index of one -- two words that a
//    list pass does not otherwise use);
//  * what a batch passes on is gathered in LDS and appended with one global atomic per block and batch: appends are single-address
//    returning atomics, ~87 per microsecond chip-wide, so one per wave or per entry would bound the kernel.
// The counts are exact when the output list is too small (stores are clipped): the host grows it and repeats the pass.
// =============================================================================================
constexpr int kPairsBlock = kAppendBlock;
constexpr unsigned kPairsMaxGrid = 1024;
constexpr int kPairsSteps = 8;                 // pairs_direct_kernel: 16-bucket steps whose loads are in flight together

template <class Rec>                        // (the record type of what the kernel passes on, as for BlockAppendLdsT)
struct PairsLdsT {
    BlockAppendLdsT<Rec> app;               // (block_append, common.cuh; app.cand = the batch's entries with an equal band signature)
    uint32_t bad;
    u64 eval, bad_at;                       // the block's tallies, added up when its waves end
};
using PairsLds = PairsLdsT<selhip_int2_t>;

template <class Rec>
__device__ __forceinline__ void pairs_lds_init(PairsLdsT<Rec>& s) {
    if (threadIdx.x == 0) { block_append_reset(s.app); s.bad = 0; s.eval = 0; s.bad_at = 0; }
    __syncthreads();
}

// per-wave tallies, wave-uniform
struct PairsTally {
    u64 eval = 0, bad_at = 0;
    uint32_t bad = 0;
};

// entry j of the list (in: j is inside it), smaller rank first; *live as defined above.  Entries that are not live come back as
// {0, 0}, so that whatever the caller reads through them stays inside the arrays (n >= 1: the host launches nothing for an empty set)
__device__ __forceinline__ selhip_int2_t pairs_entry(const selhip_int2_t* __restrict__ list, u64 j, bool in, int n,
                                                     const u64* __restrict__ ecard, double tau, int use_cb, PairsTally& tl, bool* live) {
    int x = 0, y = 0;
    if (in) {
        const int2 v = *reinterpret_cast<const int2*>(list + j);              // (the host checked the list's 8-byte alignment)
        x = min(v.x, v.y); y = max(v.x, v.y);
    }
    const bool valid = in && x >= 0 && y < n && x != y;
    bool ok = false;
    if (valid) {
        const u64 e_lo = ecard[x], e_hi = ecard[y];
        ok = e_hi != 0 && (!use_cb || cb_pred(tau, e_lo, e_hi));
    }
    const u64 bad_mask = __ballot(in && !valid);
    tl.eval += (u64)__popcll(__ballot(ok));
    if (bad_mask) {
        tl.bad += (uint32_t)__popcll(bad_mask);
        tl.bad_at = j - (u64)(threadIdx.x & (kWave - 1)) + (u64)(63 - __builtin_clzll(bad_mask)) + 1;      // later batches have larger indices
    }
    *live = ok;
    selhip_int2_t pr;
    pr.x = ok ? x : 0; pr.y = ok ? y : 0;
    return pr;
}

// the block's tallies into the pass's counter block 0
template <class Rec>
__device__ __forceinline__ void pairs_block_tally(PairsLdsT<Rec>& s, const PairsTally& tl, int lane, PassCounters* __restrict__ pc0) {
    if (lane == 0) {
        if (tl.eval) atomicAdd(&s.eval, tl.eval);
        if (tl.bad) { atomicAdd(&s.bad, tl.bad); atomicMax(&s.bad_at, tl.bad_at); }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (s.eval) atomicAdd(&pc0->n_evaluated, s.eval);
        if (s.bad) { atomicAdd(&pc0->n_pre, (u64)s.bad); atomicMax(&pc0->n_pre_segmax, s.bad_at); }
    }
}

// ---------------------------------------------------------------------------------------------
// pairs_filter_kernel: one lane per entry of list[off, end).  The live entries go on as they are (smaller rank first): the whole of
// stage 1 for the criteria without an smh_a stage -- hll_a / hll_an take them window by window, criterion none all at once.
// Resources (compiler's report for gfx950, -O3): 30 VGPRs, no scratch, 4 136 B of LDS; occupancy 8 waves per SIMD.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPairsBlock)
void pairs_filter_kernel(const selhip_int2_t* __restrict__ list, u64 off, u64 end, int n, const u64* __restrict__ ecard, double tau, int use_cb,
                         selhip_int2_t* __restrict__ out, u64 out_cap, u64* __restrict__ out_count, PassCounters* __restrict__ pc0) {
    __shared__ PairsLds s;
    const int lane = threadIdx.x & (kWave - 1);
    pairs_lds_init(s);
    PairsTally tl;
    for (u64 base = off + (u64)blockIdx.x * kPairsBlock; base < end; base += (u64)gridDim.x * kPairsBlock) {
        const u64 j = base + threadIdx.x;
        bool live;
        const selhip_int2_t pr = pairs_entry(list, j, j < end, n, ecard, tau, use_cb, tl, &live);
        block_append(s.app, live, pr, lane, out, out_cap, out_count, nullptr);
    }
    pairs_block_tally(s, tl, lane, pc0);
}

// ---------------------------------------------------------------------------------------------
// pairs_verify_kernel: the signature route.  verify16_kernel with the list, not the join's 64 append segments, as its input: the
// body is verify16_batch (kernel_verify.cuh) -- an entry with a signature bit set is a CANDIDATE (counted in n_candidates) -- and
// sig_candidate_ok decides it (`force_fallback`: test hook "verify_fb").
// Resources (compiler's report for gfx950, -O3): 126 VGPRs (verify16_batch keeps 16 signature loads in flight), 94 SGPRs, no scratch,
// no spills, 4 136 B of LDS; occupancy 4 waves per SIMD.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPairsBlock)
void pairs_verify_kernel(const u64* __restrict__ aux, int m, int n_rows, int n_bands, const uint32_t* __restrict__ sigQ,
                         const selhip_int2_t* __restrict__ list, u64 n_pairs, int n, const u64* __restrict__ ecard, double tau, int use_cb,
                         selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, PassCounters* __restrict__ pc0,
                         int force_fallback) {
    __shared__ PairsLds s;
    const int lane = threadIdx.x & (kWave - 1);
    pairs_lds_init(s);
    PairsTally tl;
    for (u64 base = (u64)blockIdx.x * kPairsBlock; base < n_pairs; base += (u64)gridDim.x * kPairsBlock) {
        const u64 j = base + threadIdx.x;
        bool live;
        const selhip_int2_t pr = pairs_entry(list, j, j < n_pairs, n, ecard, tau, use_cb, tl, &live);
        const Verify16Masks vm = verify16_batch(aux, m, n_rows, n_bands, sigQ, pr, __ballot(live), lane);
        bool ok = false;
        if ((vm.has >> lane) & 1ull)
            ok = sig_candidate_ok((vm.eq >> lane) & 1ull, force_fallback, aux + (long long)pr.x * m, aux + (long long)pr.y * m, n_rows, n_bands);
        if (lane == 0 && vm.has) atomicAdd(&s.app.cand, (uint32_t)__popcll(vm.has));
        block_append(s.app, ok, pr, lane, surv, surv_cap, &pc->n_survivors, &pc->n_candidates);
    }
    pairs_block_tally(s, tl, lane, pc0);
}

// ---------------------------------------------------------------------------------------------
// pairs_direct_kernel: the direct route, for ANY band shape with n_rows * n_bands = m.  16 lanes per entry again; a step compares
// 16 consecutive buckets of both rows (128 contiguous bytes per row) and the quarter-wave's share of the ballot is a 16-bit equality
// mask.  The band test runs on that bit string with integer operations whose operands other than the mask are wave-uniform: the
// bands that a step closes are tested against their bit ranges, and a band that straddles steps carries "equal so far" in `carry`.
// kPairsSteps steps' loads (128 buckets of both rows) are in flight together; an entry stops loading at the first such group that
// closed a fully equal band.
// gpw = groups of four entries a wave works through per batch, one after the other (1 .. 16; pairs_groups_per_wave): a group is
// m / 128 dependent memory round trips, so a short list is spread over as many waves as it has groups and a long one fills the
// wave slots with 16 groups each.  (With 16 groups for every length a list of 1 250 entries took 0.31 ms on 24 waves, three times
// the lane-per-pair kernel it replaced in the launchers: profiles/pairlist_bench.json has the figures before and after.)
// LAUNCHER: the form of the drop-in launchers (abi_compat.inc) -- the truncated cards come from `cards` on the fly, the entry keeps
// its orientation (x's card over y's in the CB ratio, like the reference's kernels) and no rank is checked, because the reference's
// parameter list carries no genome count; nothing is tallied.
// Resources (compiler's report for gfx950, -O3): context form 58 VGPRs, launcher form 56; no scratch, 4 136 B of LDS; occupancy
// 8 waves per SIMD.
// ---------------------------------------------------------------------------------------------
template <bool LAUNCHER>
__global__ __launch_bounds__(kPairsBlock)
void pairs_direct_kernel(const u64* __restrict__ aux, int m, int n_rows, int n_bands,
                         const selhip_int2_t* __restrict__ list, u64 n_pairs, int n, const u64* __restrict__ ecard,
                         const double* __restrict__ cards, double tau, int use_cb, int gpw,
                         selhip_int2_t* __restrict__ surv, u64 surv_cap, u64* __restrict__ surv_count, PassCounters* __restrict__ pc0) {
    __shared__ PairsLds s;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sub = lane & 15, quarter = lane >> 4, qshift = quarter * 16;
    const int per_wave = 4 * gpw;                                             // entries a wave takes per batch: its first per_wave lanes hold one each
    const u64 per_block = (u64)(kPairsBlock / kWave) * per_wave;
    pairs_lds_init(s);
    PairsTally tl;
    for (u64 base = (u64)blockIdx.x * per_block; base < n_pairs; base += (u64)gridDim.x * per_block) {
        const u64 j = base + (u64)(wave * per_wave + lane);
        const bool in = lane < per_wave && j < n_pairs;
        bool live;
        selhip_int2_t pr;
        if constexpr (LAUNCHER) {
            pr.x = 0; pr.y = 0;
            live = in;
            if (live) {
                const int2 v = *reinterpret_cast<const int2*>(list + j);
                const u64 e1 = selhip::trunc_card(cards[v.x]), e2 = selhip::trunc_card(cards[v.y]);
                live = e2 != 0 && (!use_cb || cb_pred(tau, e1, e2));          // selection.cpp:281-282
                if (live) { pr.x = v.x; pr.y = v.y; }
            }
        } else {
            pr = pairs_entry(list, j, in, n, ecard, tau, use_cb, tl, &live);
        }
        const u64 live_mask = __ballot(live);
        u64 ok_mask = 0;
#pragma unroll 1
        for (int t = 0; t < gpw; ++t) {
            if (((live_mask >> (t * 4)) & 0xFull) == 0) continue;             // none of this group's four entries is live
            const int src = t * 4 + quarter;
            const int px = __shfl(pr.x, src, kWave), py = __shfl(pr.y, src, kWave);
            const u64* __restrict__ a = aux + (long long)px * m;
            const u64* __restrict__ b = aux + (long long)py * m;
            bool open = (live_mask >> src) & 1ull;                            // my quarter's entry is still looking for an equal band
            bool found = false, carry = true;
            int band_start = 0;                                               // first bucket of the first band no step has closed (wave-uniform)
#pragma unroll 1
            for (int p0 = 0; p0 < m; p0 += 16 * kPairsSteps) {
                u64 va[kPairsSteps], vb[kPairsSteps];
#pragma unroll
                for (int u = 0; u < kPairsSteps; ++u) {
                    const int idx = p0 + u * 16 + sub;
                    const bool ld = open && idx < m;
                    va[u] = ld ? a[idx] : 0ull;
                    vb[u] = ld ? b[idx] : 1ull;
                }
#pragma unroll
                for (int u = 0; u < kPairsSteps; ++u) {
                    const int q0 = p0 + u * 16;
                    const uint32_t e = (uint32_t)(__ballot(va[u] == vb[u]) >> qshift) & 0xFFFFu;
                    const int q_end = min(q0 + 16, m);
                    while (band_start < q_end) {
                        const int lo = max(band_start, q0) - q0, hi = min(band_start + n_rows, q_end) - q0;
                        const uint32_t seg = ((1u << (hi - lo)) - 1u) << lo;
                        const bool eq = (band_start < q0 ? carry : true) && (e & seg) == seg;
                        if (band_start + n_rows > q_end) { carry = eq; break; }          // the band goes on in the next step
                        found |= eq;
                        band_start += n_rows;
                    }
                }
                open = open && !found;
                if (__ballot(open) == 0) break;
            }
            ok_mask |= pairs_quarter_bits(__ballot(found && sub == 0), t * 4);
        }
        const bool ok = (ok_mask >> lane) & 1ull;
        block_append(s.app, ok, pr, lane, surv, surv_cap, surv_count, nullptr);
    }
    if constexpr (!LAUNCHER) pairs_block_tally(s, tl, lane, pc0);
}

// ---------------------------------------------------------------------------------------------
// pairs_count_kernel: stage 1 of criterion smh_c (kernel_smhc.cuh) over a list.  pairs_direct_kernel's shape -- 16 lanes per entry,
// groups of four entries, gpw groups per wave and batch, kPairsSteps 16-bucket steps' loads in flight together -- with the count over
// ALL m buckets in place of the band test: every step adds the population count of the quarter-wave's 16-bit equality mask, and
// smhc_selects decides the entry when its row is through.  Nothing stops early: a count needs every bucket.
// RULE = kSmhcContainment (kernel_smhc.cuh): the entry's own exact threshold in place of c_min, from the cardinalities of its two ranks.
// EMIT (kernel_smhc.cuh; false = the kernel as it was, instruction for instruction): every group hands its four counts to the lanes
// that hold the entries; an entry that passed the count test is tallied in *surv_count -- not stored -- and its record {x, y, V},
// V = selhip::smh_value(...) >= tau, goes into the result list `surv` behind pc0->n_results through the same block append.
// ---------------------------------------------------------------------------------------------
struct PairsGammaEmit { double gamma; SmhcEmit em; };              // (the emit form's last argument: gamma, and SmhcEmit behind it)
template <bool EMIT> using PairsGammaArg = std::conditional_t<EMIT, PairsGammaEmit, double>;
__device__ __forceinline__ double pairs_gamma(double g) { return g; }
__device__ __forceinline__ double pairs_gamma(const PairsGammaEmit& g) { return g.gamma; }

template <int RULE, bool EMIT = false>
__global__ __launch_bounds__(kPairsBlock)
void pairs_count_kernel(const u64* __restrict__ aux, int m, int c_min,
                        const selhip_int2_t* __restrict__ list, u64 n_pairs, int n, const u64* __restrict__ ecard, double tau, int use_cb, int gpw,
                        SmhcRecord<EMIT>* __restrict__ surv, u64 surv_cap, u64* __restrict__ surv_count, PassCounters* __restrict__ pc0,
                        PairsGammaArg<EMIT> gamma) {
    __shared__ PairsLdsT<SmhcRecord<EMIT>> s;
    __shared__ u64 s_passed;                                                  // EMIT: the block's entries that passed the count test
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    const int sub = lane & 15, quarter = lane >> 4, qshift = quarter * 16;
    const int per_wave = 4 * gpw;                                             // entries a wave takes per batch: its first per_wave lanes hold one each
    const u64 per_block = (u64)(kPairsBlock / kWave) * per_wave;
    if constexpr (EMIT) { if (threadIdx.x == 0) s_passed = 0; }               // (before the barrier of pairs_lds_init)
    pairs_lds_init(s);
    PairsTally tl;
    for (u64 base = (u64)blockIdx.x * per_block; base < n_pairs; base += (u64)gridDim.x * per_block) {
        const u64 j = base + (u64)(wave * per_wave + lane);
        const bool in = lane < per_wave && j < n_pairs;
        bool live;
        const selhip_int2_t pr = pairs_entry(list, j, in, n, ecard, tau, use_cb, tl, &live);
        const u64 live_mask = __ballot(live);
        u64 ok_mask = 0;
        int my_cnt = 0;                                                       // EMIT: the count of the entry this lane holds
#pragma unroll 1
        for (int t = 0; t < gpw; ++t) {
            if (((live_mask >> (t * 4)) & 0xFull) == 0) continue;             // none of this group's four entries is live
            const int src = t * 4 + quarter;
            const int px = __shfl(pr.x, src, kWave), py = __shfl(pr.y, src, kWave);       // (entries that are not live: {0, 0}, inside the arrays)
            const u64* __restrict__ a = aux + (long long)px * m;
            const u64* __restrict__ b = aux + (long long)py * m;
            const bool open = (live_mask >> src) & 1ull;
            int cnt = 0;                                                      // my quarter's count
#pragma unroll 1
            for (int p0 = 0; p0 < m; p0 += 16 * kPairsSteps) {
                u64 va[kPairsSteps], vb[kPairsSteps];
#pragma unroll
                for (int u = 0; u < kPairsSteps; ++u) {
                    const int idx = p0 + u * 16 + sub;
                    const bool ld = open && idx < m;
                    va[u] = ld ? a[idx] : 0ull;
                    vb[u] = ld ? b[idx] : 1ull;
                }
#pragma unroll
                for (int u = 0; u < kPairsSteps; ++u)
                    cnt += __popc((uint32_t)(__ballot(va[u] == vb[u]) >> qshift) & 0xFFFFu);
            }
            int thr = c_min;
            if constexpr (RULE == kSmhcContainment) thr = smhc_pair_threshold(m, pairs_gamma(gamma), ecard[px], ecard[py], c_min);       // ({0, 0} when not live)
            ok_mask |= pairs_quarter_bits(__ballot(open && sub == 0 && smhc_selects(cnt, thr)), t * 4);
            if constexpr (EMIT) {
                const int c4 = __shfl(cnt, (lane & 3) * 16, kWave);           // lane 4 t + j holds the entry of quarter j
                if ((lane >> 2) == t) my_cnt = c4;
            }
        }
        const bool ok = (ok_mask >> lane) & 1ull;
        if constexpr (EMIT) {
            bool sel;
            const selhip_pair_t r = smhc_record(gamma.em, m, my_cnt, ecard[pr.x], ecard[pr.y], pr.x, pr.y, &sel);      // ({0, 0} when not live)
            const u64 okb = __ballot(ok);
            if (okb && lane == 0) atomicAdd(&s_passed, (u64)__popcll(okb));
            block_append(s.app, ok && sel, r, lane, surv, surv_cap, &gamma.em.pc0->n_results, nullptr);
        } else {
            block_append(s.app, ok, pr, lane, surv, surv_cap, surv_count, nullptr);
        }
    }
    pairs_block_tally(s, tl, lane, pc0);
    if constexpr (EMIT) {                                                     // (behind the tally's barrier)
        if (threadIdx.x == 0 && s_passed) atomicAdd(surv_count, s_passed);
    }
}

}  // namespace

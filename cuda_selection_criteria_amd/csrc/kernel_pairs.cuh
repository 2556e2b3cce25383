// kernel_pairs.cuh -- stage 1 of the pair-list passes (selhip_ctx_run_pairs, host_pairs.hpp): the pair space is a caller's list of
// entries {x, y}, not a triangle or a rectangle that the pass enumerates itself.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
#pragma once

namespace {

// =============================================================================================
// What the three kernels share.  A block takes kPairsBlock consecutive entries per batch:
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
constexpr int kPairsBlock = 512;
constexpr unsigned kPairsMaxGrid = 1024;
constexpr int kPairsSteps = 8;                 // pairs_direct_kernel: 16-bucket steps whose loads are in flight together

struct PairsLds {
    selhip_int2_t out[kPairsBlock];
    u64 base;
    uint32_t count, cand;                   // this batch: entries passed on, entries with an equal band signature
    uint32_t bad;
    u64 eval, bad_at;                       // the block's tallies, added up when its waves end
};

__device__ __forceinline__ void pairs_lds_init(PairsLds& s) {
    if (threadIdx.x == 0) { s.count = 0; s.cand = 0; s.bad = 0; s.eval = 0; s.bad_at = 0; }
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

// block-uniform: the batch's entries with `ok` go to out[] behind *out_count; cand_count (if given) takes the batch's s.cand
__device__ __forceinline__ void pairs_block_append(PairsLds& s, bool ok, selhip_int2_t pr, int lane, selhip_int2_t* __restrict__ out, u64 out_cap,
                                                   u64* __restrict__ out_count, u64* __restrict__ cand_count) {
    const u64 okb = __ballot(ok);
    if (okb) {
        uint32_t wbase = 0;
        if (lane == 0) wbase = atomicAdd(&s.count, (uint32_t)__popcll(okb));
        wbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)wbase);
        if (ok) s.out[wbase + (uint32_t)__popcll(okb & ((1ull << lane) - 1ull))] = pr;
    }
    __syncthreads();
    const uint32_t cnt = s.count;
    if (threadIdx.x == 0) {
        if (cnt) s.base = atomicAdd(out_count, (u64)cnt);
        if (cand_count && s.cand) atomicAdd(cand_count, (u64)s.cand);
    }
    __syncthreads();
    if (threadIdx.x < cnt) {
        const u64 dst = s.base + threadIdx.x;
        if (dst < out_cap) out[dst] = s.out[threadIdx.x];
    }
    __syncthreads();
    if (threadIdx.x == 0) { s.count = 0; s.cand = 0; }
    __syncthreads();
}

// the block's tallies into the pass's counter block 0
__device__ __forceinline__ void pairs_block_tally(PairsLds& s, const PairsTally& tl, int lane, PassCounters* __restrict__ pc0) {
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

// bit q of the result = the ballot's bit of lane 16 q (one bit per quarter-wave), moved up by `sh`
__device__ __forceinline__ u64 pairs_quarter_bits(u64 m, int sh) {
    return (((m >> 0) & 1ull) | (((m >> 16) & 1ull) << 1) | (((m >> 32) & 1ull) << 2) | (((m >> 48) & 1ull) << 3)) << sh;
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
        pairs_block_append(s, live, pr, lane, out, out_cap, out_count, nullptr);
    }
    pairs_block_tally(s, tl, lane, pc0);
}

// ---------------------------------------------------------------------------------------------
// pairs_verify_kernel: the signature route.  The body of verify16_kernel (kernel_sigjoin.cuh) with the list, not the join's 64 append
// segments, as its input: a wave works on its 64 entries four at a time, 16 lanes per entry; the two genomes' 32-bit signature rows
// come from the genome-major copy sigQ by 16-byte loads and give one bit per band; an entry with a bit set is a CANDIDATE (counted
// in n_candidates); its first flagged band is compared on the full sketches; equal -> survivor, not equal (a signature collision,
// or `force_fallback`) -> the literal smh_a_lane decides.
// A SECOND COPY of that body, on purpose: verify16_kernel is on the path of every all-pairs pass, and handing both kernels one
// __device__ function was not shown to leave its ISA as it is.  A change of the rule "signature equal, band not equal" belongs in
// both (and in the four other places DESIGN.md section 4.2b lists).
// Resources (compiler's report for gfx950, -O3): 73 VGPRs, no scratch, 4 136 B of LDS; occupancy 6 waves per SIMD.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kPairsBlock)
void pairs_verify_kernel(const u64* __restrict__ aux, int m, int n_rows, int n_bands, const uint32_t* __restrict__ sigQ,
                         const selhip_int2_t* __restrict__ list, u64 n_pairs, int n, const u64* __restrict__ ecard, double tau, int use_cb,
                         selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, PassCounters* __restrict__ pc0,
                         int force_fallback) {
    __shared__ PairsLds s;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & 15, quarter = lane >> 4, qshift = quarter * 16;
    const int nq = n_bands >> 2;                                              // 16-byte groups per genome (n_bands % 8 == 0, <= 32)
    pairs_lds_init(s);
    PairsTally tl;
    for (u64 base = (u64)blockIdx.x * kPairsBlock; base < n_pairs; base += (u64)gridDim.x * kPairsBlock) {
        const u64 j = base + threadIdx.x;
        bool live;
        const selhip_int2_t pr = pairs_entry(list, j, j < n_pairs, n, ecard, tau, use_cb, tl, &live);
        const u64 live_mask = __ballot(live);
        u64 has_mask = 0, ok_mask = 0;                                        // bit p: entry p of this wave's 64 (wave-uniform)
#pragma unroll 1
        for (int s0 = 0; s0 < 16; s0 += 8) {
            int px[8], py[8];
            uint32_t lm[8];           // bit t (0..3): band 4*sub+t equal; bit 4+t: band 4*(sub+16)+t equal
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const int src = (s0 + t) * 4 + quarter;
                px[t] = __shfl(pr.x, src, kWave);
                py[t] = __shfl(pr.y, src, kWave);
                const uint4* a = reinterpret_cast<const uint4*>(sigQ + (long long)px[t] * n_bands);
                const uint4* b = reinterpret_cast<const uint4*>(sigQ + (long long)py[t] * n_bands);
                uint32_t bits = 0;
                if (sub < nq) {
                    const uint4 u = a[sub], v = b[sub];
                    bits |= (u.x == v.x ? 1u : 0u) | (u.y == v.y ? 2u : 0u) | (u.z == v.z ? 4u : 0u) | (u.w == v.w ? 8u : 0u);
                }
                if (sub + 16 < nq) {
                    const uint4 u = a[sub + 16], v = b[sub + 16];
                    bits |= (u.x == v.x ? 16u : 0u) | (u.y == v.y ? 32u : 0u) | (u.z == v.z ? 64u : 0u) | (u.w == v.w ? 128u : 0u);
                }
                lm[t] = ((live_mask >> src) & 1ull) ? bits : 0u;
            }
#pragma unroll
            for (int t = 0; t < 8; ++t) {
                const uint32_t mine = (uint32_t)(__ballot(lm[t] != 0u) >> qshift) & 0xFFFFu;   // lanes of my quarter with a bit
                const bool has = mine != 0u;
                const int src_sub = has ? __builtin_ctz(mine) : 0;
                const uint32_t lmv = (uint32_t)__shfl((int)lm[t], qshift + src_sub, kWave);
                const int bt = has ? __builtin_ctz(lmv) : 0;
                const int band = bt < 4 ? src_sub * 4 + bt : (src_sub + 16) * 4 + (bt - 4);
                const u64* x = aux + (long long)px[t] * m + (long long)band * n_rows;
                const u64* y = aux + (long long)py[t] * m + (long long)band * n_rows;
                bool eq = true;
                for (int j0 = sub; j0 < n_rows; j0 += 16)
                    if (has) eq &= x[j0] == y[j0];
                const bool all_eq = ((uint32_t)(__ballot(eq) >> qshift) & 0xFFFFu) == 0xFFFFu && !force_fallback;
                const int sh = (s0 + t) * 4;
                has_mask |= pairs_quarter_bits(__ballot(has && sub == 0), sh);
                ok_mask |= pairs_quarter_bits(__ballot(has && all_eq && sub == 0), sh);
            }
        }
        const u64 fb_mask = has_mask & ~ok_mask;                              // signature collision: the literal predicate decides
        bool ok = (ok_mask >> lane) & 1ull;
        if ((fb_mask >> lane) & 1ull) ok = smh_a_lane(aux + (long long)pr.x * m, aux + (long long)pr.y * m, n_rows, n_bands);
        if (lane == 0 && has_mask) atomicAdd(&s.cand, (uint32_t)__popcll(has_mask));
        pairs_block_append(s, ok, pr, lane, surv, surv_cap, &pc->n_survivors, &pc->n_candidates);
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
        pairs_block_append(s, ok, pr, lane, surv, surv_cap, surv_count, nullptr);
    }
    if constexpr (!LAUNCHER) pairs_block_tally(s, tl, lane, pc0);
}

}  // namespace

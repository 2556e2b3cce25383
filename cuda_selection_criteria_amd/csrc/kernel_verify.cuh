// kernel_verify.cuh -- the exact verification behind every band-signature join: the literal predicate, the rule that decides a
// candidate, the 16-lanes-per-pair comparison the batched verifications share, and the two verification kernels of ALGO_SIG.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
#pragma once

namespace {

// ---------------------------------------------------------------------------------------------
// smh_a for one pair evaluated by ONE LANE (any m, rows, bands): criteria_sketch.hpp:66-81 literally.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool smh_a_lane(const u64* __restrict__ v1, const u64* __restrict__ v2,
                                           int n_rows, int n_bands) {
    for (int b = 0; b < n_bands; ++b) {
        const u64* x = v1 + (long long)b * n_rows;
        const u64* y = v2 + (long long)b * n_rows;
        int j = 0;
        while (j < n_rows && x[j] == y[j]) ++j;
        if (j == n_rows) return true;
    }
    return false;
}

// ---------------------------------------------------------------------------------------------
// THE RULE of every verification that looks at one band only.  A candidate is a pair with a band whose 32-bit signatures agree; the
// caller compared the first such band on the full sketches (`band_equal`).  An entirely equal band IS smh_a, so the pair survives.
// A band that is not equal met a signature collision (~2^-32 per band), which says nothing about the pair's other bands -- another
// band may be equal behind its own signature -- so the literal predicate on the two rows v1, v2 decides: a collision can add work,
// it can never produce or drop a pair, and the survivor set is the stream kernel's.  `force_fallback` (test hook "verify_fb")
// treats every comparison as a collision.
// Callers: verify16_kernel, pairs_verify_kernel (through verify16_batch: one lane of each pair's sixteen), the queue check of
// small_pass_kernel (lane 0 of sixteen), query_verify_kernel (one lane per match).  verify_kernel, run_emit_kernel and
// pairlist_smh_kernel take the literal predicate on every candidate.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sig_candidate_ok(bool band_equal, int force_fallback, const u64* __restrict__ v1, const u64* __restrict__ v2,
                                                 int n_rows, int n_bands) {
    if (band_equal && !force_fallback) return true;
    return smh_a_lane(v1, v2, n_rows, n_bands);
}

// One band of n_rows buckets compared by a quarter-wave (lane's 16-lane group: sub = lane & 15 takes buckets sub, sub + 16, ...);
// `on` (quarter-uniform) = the quarter has a pair, otherwise nothing is loaded.  Wave-uniformly reached; true on all sixteen lanes
// iff every bucket is equal.  The queue check of small_pass_kernel uses it (one band per quarter: nothing to batch); verify16_batch
// compares eight steps' bands at once, with unguarded loads, in its own loops.
__device__ __forceinline__ bool band_equal16(const u64* x, const u64* y, int n_rows, bool on, int lane) {
    bool eq = true;
    for (int j0 = lane & 15; j0 < n_rows; j0 += 16)
        if (on) eq &= x[j0] == y[j0];
    return ((uint32_t)(__ballot(eq) >> (lane & 48)) & 0xFFFFu) == 0xFFFFu;
}

// bit q of the result = the ballot's bit of lane 16 q (one bit per quarter-wave), moved up by `sh`
__device__ __forceinline__ u64 pairs_quarter_bits(u64 m, int sh) {
    return (((m >> 0) & 1ull) | (((m >> 16) & 1ull) << 1) | (((m >> 32) & 1ull) << 2) | (((m >> 48) & 1ull) << 3)) << sh;
}

// ---------------------------------------------------------------------------------------------
// verify16_batch: a wave's 64 pairs (lane p holds pair p in `pr`; `live_mask` = the lanes that hold one), four at a time, 16 lanes
// per pair (step s: quarter-wave q has pair 4s+q), in two half-batches of eight steps.
//  1. 32-bit signatures: the lanes of a quarter read the two genomes' signature rows from the genome-major copy sigQ
//     (coalesced 16-B loads, 2 x n_bands*4 bytes per pair, L2-resident) and keep one bit per band "32-bit signature
//     equal".  Pairs with a bit set are exactly the candidate set of the 32-bit join: mask `has`.
//  2. A band that is entirely equal has an equal signature, so only bands with a bit set can make smh_a true: the first
//     such band of each pair is compared on the full sketches (n_rows u64 per genome, 16 lanes): mask `eq` (a subset of `has`).
// Both masks are wave-uniform, bit p = pair p.  The caller hands each pair of `has` to sig_candidate_ok on its own lane.
// EVERY LOAD IS UNCONDITIONAL, at a clamped index, and the lane conditions (sub < nq, the live mask, `has`, sub < n_rows) are applied
// to the loaded bits: the compiler does not move a load out of a lane-divergent guard that also consumes it, and with the guards
// every step was a round trip of its own (s_waitcnt vmcnt(0) behind each pair of loads: ~35 dependent round trips a wave).  Now a
// half-batch issues the 16 signature loads of its eight steps back to back, then -- the bands of all eight steps known, by ballots
// and shuffles alone -- their 16 sketch loads, each group behind ONE s_waitcnt vmcnt(0) (VERIFY16_ALL_LOADED): 2 round trips a
// half-batch, 4 a batch (profiles/verify_batch_isa.txt shows the load / wait sequence of the code object before and after).  What
// makes the unguarded loads valid:
//  * a lane of a dead pair holds pr = {0, 0} (verify16_kernel, pairs_entry) and reads row 0, which exists whenever a batch runs;
//  * a lane with sub >= nq re-reads signature group nq - 1 and its bits are dropped; one with sub >= n_rows re-reads bucket
//    n_rows - 1, a duplicate of lane n_rows - 1's comparison, which cannot change the AND over the sixteen lanes;
//  * a quarter without a flagged band compares band 0 of row 0 with itself (one cache line for all such quarters, no sketch
//    traffic for the 16-bit matches that are no candidates) and is masked by `has`.
// Further round trips, both behind wave-uniform trip counts: 128 bands (nq = 32) take a second batched group of 16 signature loads,
// bands of more than 16 buckets a remainder loop of batched loads (16 per trip) over the buckets sub + 16, sub + 32, ...
// Neither the half-batch loop nor the group loop may be unrolled (the 64 registers of 16 signature loads in flight are the budget:
// 124 VGPRs in verify16_kernel), the loops over the eight steps must.
// ---------------------------------------------------------------------------------------------
struct Verify16Masks { u64 has, eq; };

// bits 0..3 of the result: the four signatures of a 16-byte group equal
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t sig_group_bits(const u32x4 u, const u32x4 v) {
    return (u.x == v.x ? 1u : 0u) | (u.y == v.y ? 2u : 0u) | (u.z == v.z ? 4u : 0u) | (u.w == v.w ? 8u : 0u);
}

// x of the lane K places up in the lane's quarter-wave (a DPP row), rotating inside it
template <int K>
__device__ __forceinline__ uint32_t quarter_ror(uint32_t x) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)x, 0x120 + K, 0xF, 0xF, true);
}

// An empty statement that takes the 16 loaded values a[0..7], b[0..7] (whole registers: u32x4 or u64) and hands them on: everything
// computed from them depends on ALL sixteen loads, so the compiler can neither start comparing after the first few and issue the
// rest behind that wait (it does, to save registers), nor sink one of them into a guard.  One s_waitcnt vmcnt(0) stands in its place.
#define VERIFY16_ALL_LOADED(a, b)                                                                                                      \
    asm volatile("" : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]),                 \
                      "+v"(b[0]), "+v"(b[1]), "+v"(b[2]), "+v"(b[3]), "+v"(b[4]), "+v"(b[5]), "+v"(b[6]), "+v"(b[7]))

__device__ __forceinline__ Verify16Masks verify16_batch(const u64* __restrict__ aux, int m, int n_rows, int n_bands, const uint32_t* __restrict__ sigQ,
                                                        selhip_int2_t pr, u64 live_mask, int lane) {
    const int sub = lane & 15, quarter = lane >> 4, qshift = quarter * 16;
    const int nq = n_bands >> 2;                                              // 16-byte groups per genome (n_bands % 8 == 0, <= 32)
    const int n_groups = nq > 16 ? 2 : 1;                                     // 128 bands: a lane has a second group, sub + 16
    const int j0 = min(sub, n_rows - 1);                                      // clamped: lanes past the band re-read its last bucket
    Verify16Masks vm{0, 0};
#pragma unroll 1
    for (int s0 = 0; s0 < 16; s0 += 8) {
        int px[8], py[8];
        uint32_t lm[8];           // bit t (0..3): band 4*sub+t equal; bit 4+t: band 4*(sub+16)+t equal
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int src = (s0 + s) * 4 + quarter;
            px[s] = __shfl(pr.x, src, kWave);
            py[s] = __shfl(pr.y, src, kWave);
            lm[s] = 0u;
        }
        // ---- phase 1: the signatures of eight steps, all 16 loads of a group before the first comparison.  The trip count is
        // wave-uniform; only 128 bands take the second trip.
#pragma unroll 1
        for (int g = 0; g < n_groups; ++g) {
            const int gi = min(sub + 16 * g, nq - 1);                         // clamped: lanes past the row re-read its last group
            // which of the loaded bits count, as an AND mask: a select here becomes a lane-divergent branch, and the compiler sinks
            // loads into it
            const uint32_t keep = sub + 16 * g < nq ? 0xFu : 0u;
            u32x4 u[8], v[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) {
                int x = px[s], y = py[s];
                asm volatile("" : "+v"(x), "+v"(y));                          // (the row addresses are formed here, not kept across the trips)
                u[s] = reinterpret_cast<const u32x4*>(sigQ + (long long)x * n_bands)[gi];
                v[s] = reinterpret_cast<const u32x4*>(sigQ + (long long)y * n_bands)[gi];
            }
            VERIFY16_ALL_LOADED(u, v);
#pragma unroll
            for (int s = 0; s < 8; ++s) lm[s] |= (sig_group_bits(u[s], v[s]) & keep) << (4 * g);
        }
        // ---- phase 2: the first flagged band of every step (ballots and shuffles only), then all their sketch loads
        uint32_t has_bits = 0, eq_bits = 0;                                   // bit s: step s (has: quarter-uniform; eq: this lane's buckets)
        long long ox[8], oy[8];                                               // the band's first bucket in aux
#pragma unroll
        for (int s = 0; s < 8; ++s) {
            const int src = (s0 + s) * 4 + quarter;
            const uint32_t lms = ((live_mask >> src) & 1ull) ? lm[s] : 0u;
            const uint32_t mine = (uint32_t)(__ballot(lms != 0u) >> qshift) & 0xFFFFu;     // lanes of my quarter with a bit
            const bool has = mine != 0u;
            const int src_sub = has ? __builtin_ctz(mine) : 0;
            const uint32_t lmv = (uint32_t)__shfl((int)lms, qshift + src_sub, kWave);
            const int t = has ? __builtin_ctz(lmv) : 0;
            const int band = t < 4 ? src_sub * 4 + t : (src_sub + 16) * 4 + (t - 4);
            has_bits |= has ? 1u << s : 0u;
            ox[s] = (long long)(has ? px[s] : 0) * m + (long long)band * n_rows;           // (no candidate: band 0 of row 0, twice)
            oy[s] = (long long)(has ? py[s] : 0) * m + (long long)band * n_rows;
        }
        {
            u64 x[8], y[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) { x[s] = aux[ox[s] + j0]; y[s] = aux[oy[s] + j0]; }
            VERIFY16_ALL_LOADED(x, y);
#pragma unroll
            for (int s = 0; s < 8; ++s) eq_bits |= x[s] == y[s] ? 1u << s : 0u;
        }
        for (int o = 16; o < n_rows; o += 16) {                               // wave-uniform trip count: bands of more than 16 buckets
            const int j = min(sub + o, n_rows - 1);
            u64 x[8], y[8];
#pragma unroll
            for (int s = 0; s < 8; ++s) { x[s] = aux[ox[s] + j]; y[s] = aux[oy[s] + j]; }
            VERIFY16_ALL_LOADED(x, y);
#pragma unroll
            for (int s = 0; s < 8; ++s) eq_bits &= x[s] == y[s] ? ~0u : ~(1u << s);
        }
        // a band is equal iff its sixteen lanes are: AND over the quarter (a DPP row), all eight steps at once
        uint32_t ok_bits = eq_bits;
        ok_bits &= quarter_ror<1>(ok_bits);
        ok_bits &= quarter_ror<2>(ok_bits);
        ok_bits &= quarter_ror<4>(ok_bits);
        ok_bits &= quarter_ror<8>(ok_bits);
        ok_bits &= has_bits;
        // bit p of the half-batch's masks = pair p = step p >> 2 of quarter p & 3: lane p (< 32) fetches that quarter's word, and a
        // ballot over its bit p >> 2 lines the 32 pairs up
        const int from = (lane & 3) * 16, step = (lane >> 2) & 7;
        const uint32_t has_q = (uint32_t)__shfl((int)has_bits, from, kWave), ok_q = (uint32_t)__shfl((int)ok_bits, from, kWave);
        vm.has |= (u64)(uint32_t)__ballot(lane < 32 && ((has_q >> step) & 1u)) << (s0 * 4);
        vm.eq |= (u64)(uint32_t)__ballot(lane < 32 && ((ok_q >> step) & 1u)) << (s0 * 4);
    }
    return vm;
}

// verify_kernel: the literal smh_a on every candidate (one lane per candidate), survivors compacted.
__global__ __launch_bounds__(kBlock)
void verify_kernel(const u64* __restrict__ aux, int m, int n_rows, int n_bands,
                   const selhip_int2_t* __restrict__ cand, const u64* __restrict__ n_cand_dev, u64 cand_cap,
                   selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc) {
    u64 n_cand = *n_cand_dev;
    if (n_cand > cand_cap) n_cand = cand_cap;
    for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < n_cand; j += (u64)gridDim.x * kBlock) {
        const selhip_int2_t pr = cand[j];
        if (smh_a_lane(aux + (long long)pr.x * m, aux + (long long)pr.y * m, n_rows, n_bands)) {
            u64 idx = atomicAdd(&pc->n_survivors, 1ull);
            if (idx < surv_cap) surv[idx] = pr;
        }
    }
}

// (Round 3 built and measured the alternative of verifying INSIDE the join: every wave of sigl_join_kernel checked its own 16-bit matches
// at its end -- the candidate registers are free there -- and a light kernel compacted the survivors; bit-identical in all 90 parity tests.
// It lost: cfg3 join 101 -> 128 us for a verification 25 -> 7 us (step 0.250 -> 0.261 ms), cfg2 join 12.5 -> 26.5 us, cfg4 even
// (gpurun_out/r03/f_jv*).  A wave meets ~8 matches, so its own verification is two or three dependent memory round trips for a
// handful of pairs -- 6-8 us added to a 45 us wave that holds one of the 8 192 slots the second round of waves is waiting for -- and
// keeping the row loop at 64 registers beside it cost spills.  The separate kernel stays.)
// verify16_kernel: verification behind the 16-bit join.  A wave takes 64 pairs of the join's output at a time through verify16_batch
// (pairs with a signature bit = the candidate set of the 32-bit join, counted in n_candidates) and sig_candidate_ok.
// Recorded alternatives: a separate filter kernel appending the passing pairs to a list (58 us at cfg3 -- one
// single-address atomic per wave, ~85 of those per microsecond); one lane per pair for step 1 (uncoalesced loads: cfg4
// verification 90 -> 370 us); literal check in place on each batch's few passing lanes (cfg4 355 us) or on lanes packed
// through LDS (cfg4 205 us, cfg3 60 us).
// Output: the survivors of a block's 512 pairs (256: 27 us, 512: 24 us, 1024: 26 us at cfg3) are gathered in LDS and appended with ONE global atomic per block and
// batch (plus one for the candidate tally; block_append, common.cuh): appends are single-address atomics, ~85 per microsecond on
// this part, and a per-wave append (1 500 waves at cfg3) costs more than the whole check (52 us vs 15 us).
// force_fallback (test hook): treat every first-band comparison as a collision.
// Resources (compiler's report for gfx950, -O3): 124 VGPRs (64 of them the 16 signature loads a half-batch keeps in flight), 90 SGPRs,
// no scratch, no spills, 4 112 B of LDS; occupancy 4 waves per SIMD.  With the guarded loads it had 71 VGPRs and 7 waves, and took
// 22.6 us a launch at cfg3 against 13.8 us now; cfg4 and cfg5, where it verifies over a million matches and occupancy could matter,
// are 2 % and 1.5 % faster a step (profiles/verify_batch_ab.txt).
constexpr int kVerifyBlock = kAppendBlock;

__global__ __launch_bounds__(kVerifyBlock)
void verify16_kernel(const u64* __restrict__ aux, int m, int n_rows, int n_bands, const uint32_t* __restrict__ sigQ,
                     const selhip_int2_t* __restrict__ pre_all, const u64* __restrict__ seg_cnt, u64 pre_cap,
                     selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc, int force_fallback,
                     int* __restrict__ row_cnt, int* __restrict__ row_lab, int n) {
    __shared__ BlockAppendLds s;
    // the join's output comes in kAppendSegs lists; block b works on list b % kAppendSegs (gridDim.x is a multiple of kAppendSegs)
    const int seg = blockIdx.x % kAppendSegs;
    const u64 seg_cap = pre_cap / kAppendSegs;
    const selhip_int2_t* __restrict__ pre = pre_all + (size_t)seg * seg_cap;
    const u64 n_seg = seg_cnt[seg * kSegStride];
    if (blockIdx.x < kAppendSegs && threadIdx.x == 0 && n_seg) {             // exact totals for the host (overflow test, statistics)
        atomicAdd(&pc->n_pre, n_seg);
        atomicMax(&pc->n_pre_segmax, n_seg);
    }
    const u64 n_pre = n_seg > seg_cap ? seg_cap : n_seg;
    const int lane = threadIdx.x & (kWave - 1);
    if (threadIdx.x == 0) block_append_reset(s);
    __syncthreads();
    for (u64 base = (u64)(blockIdx.x / kAppendSegs) * kVerifyBlock; base < n_pre; base += (u64)(gridDim.x / kAppendSegs) * kVerifyBlock) {
        const u64 j = base + threadIdx.x;
        const bool live = j < n_pre;
        selhip_int2_t pr{0, 0};
        if (live) pr = pre[j];
        const Verify16Masks vm = verify16_batch(aux, m, n_rows, n_bands, sigQ, pr, __ballot(live), lane);
        bool ok = false;
        if ((vm.has >> lane) & 1ull)
            ok = sig_candidate_ok((vm.eq >> lane) & 1ull, force_fallback, aux + (long long)pr.x * m, aux + (long long)pr.y * m, n_rows, n_bands);
        if (lane == 0 && vm.has) atomicAdd(&s.cand, (uint32_t)__popcll(vm.has));
        block_append(s, ok, pr, lane, surv, surv_cap, &pc->n_survivors, &pc->n_candidates, [&](selhip_int2_t q) {
            if (row_cnt) atomicAdd(&row_cnt[q.x], 1);                        // stage 2 grouping: survivors per query row, STORED ones only
            if (row_lab) atomicMax(&row_lab[q.y], n - q.x);                  // ... and every row's smallest partner (csr_label_* in kernel_hll.cuh)
        });                                                                  //   (like csr_count_kernel: the offsets must stay inside `grouped`)
    }
}

}  // namespace

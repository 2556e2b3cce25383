// kernel_dense.cuh -- criterion "none" (SELHIP_CRIT_NONE): EVERY pair of the pass's pair space goes to the HLL-14 Jaccard test.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
//
// The pair space is what cb_bounds_kernel (all-pairs: k in [max(i + 1, z0), hi(i)]) or query_windows_kernel (queries: d in
// [lo(q), hi(q)]) leaves; nothing filters it, so stage 2 runs for all of it -- 5e7 pairs at 10 000 genomes where smh_a hands over ~9 000.
// dense_select_kernel does that in ONE launch: no pair list, no 256-byte histogram per pair in HBM, no estimator kernel behind it.
//   * unit = a tile of four neighbouring rows (one per wave of the block) x a span of kDenseSpan = 64 consecutive candidates, at
//     absolute candidate positions, so that the four waves read the SAME candidates; a wave whose row's range misses the span leaves;
//   * spans are dealt to the XCDs round robin (block b works on XCD b % 8): the blocks resident on one XCD walk neighbouring row
//     tiles against one span, whose 64 x NB x 2 KiB of planes are fetched from beyond L2 once per sweep of the rows, not once per pair,
//     and all eight XCDs are at spans of the same length at the same time (the triangle's columns grow with the span index);
//   * per candidate: bs_load + bs_pair_hist with kp from the two rows' largest register values -- the arithmetic of
//     hll_union_hist_bs_kernel<NB, 0> -- after which the even lanes hold the packed totals of the 32 bin pairs and store them into
//     column (candidate - span start) of the wave's LDS tile [32 bin pairs][64 columns];
//   * after the span, lane = candidate: the Ertl estimator on its own column, J from the truncated cards, J >= tau, and one atomic per
//     wave with a selected pair appends the records (exact count, clipped stores: the convention of ertl_select_kernel<FMA, 1>).
// The row's planes are loaded per unit and are dead before the estimator starts: its f64 state never sits next to 2 x 8 NB plane
// registers, so no instantiation spills.
// The tile's pitch is 65 dwords, not 64: the 32 storing lanes of a candidate write 32 different bin pairs of ONE column, which at
// pitch 64 is one LDS bank 32 times over; at 65 they and the estimator's reads (64 columns of one bin pair) are conflict-free.
#pragma once

namespace {

constexpr int kDenseSpan = kWave;               // candidates per unit: one per lane of the estimator
constexpr int kDensePitch = kWave + 1;          // dwords between two bin pairs of the tile

// one sketch set as the kernel reads it: bit planes, largest register value per genome, truncated cards
struct DenseSet {
    const uint32_t* bs;
    const uint8_t* gmax;
    const u64* ecard;
};

// a lane's column of the tile: bin k in half k & 1 of word k >> 1 (the packing of bs_pair_hist's totals)
struct DenseColumn {
    const uint32_t* base;       // &tile[lane]
    __device__ __forceinline__ uint32_t operator[](int k) const { return (base[(k >> 1) * kDensePitch] >> ((k & 1) << 4)) & 0xFFFFu; }
};

// the estimate of the lane's column, out of line: the estimator's f64 state and constants then get registers of their own instead of
// being allocated around the 2 x 8 NB plane registers and 24 counters of the candidate loop (inlined, <NB = 5> spilled 5 VGPRs)
template <bool FMA>
__device__ __attribute__((noinline)) double dense_estimate(const uint32_t* col, double relerr_scaled) {
    const DenseColumn c{col};
    return selhip::ertl_ml_estimate<FMA>(c, 14u, 50u, relerr_scaled);
}

// X = the rows (genomes i of an all-pairs pass, queries of a query pass), Y = the candidates (n_y of them).
// lo == nullptr: all-pairs -- row i takes k in [max(i + 1, z0), min(hi[i], n_y - 1)], z0 from pc_in (cb_bounds_kernel: first rank with
// e != 0, raised to the pass's candidate_begin); else a query pass -- row q takes d in [lo[q], hi[q]] (query_windows_kernel).
// Block b of the n_units = 8 x n_tiles x (groups of 8 spans): XCD slot x = b % 8, j = b / 8 -> row tile j % n_tiles of span
// span_base + 8 (j / n_tiles) + x.  Records: {row, candidate, value} with the ranks of their own sets; value = J, or under
// MEAS = SELHIP_MEASURE_MAX_CONTAINMENT (selhip_ctx_set_measure) I / min(e_row, e_candidate) -- selhip::pair_value either way.
template <int NB, bool FMA, int MEAS>
__global__ __launch_bounds__(kBlock, NB <= 5 ? 4 : 2)
void dense_select_kernel(DenseSet X, DenseSet Y, int n_y, const int* __restrict__ lo, const int* __restrict__ hi,
                         const PassCounters* __restrict__ pc_in, RowMap rm, int n_tiles, int span_base, long long n_units,
                         double tau, double relerr_scaled, selhip_pair_t* __restrict__ results, u64 results_cap,
                         PassCounters* __restrict__ pc) {
    __shared__ uint32_t tile_all[kWavesPerBlock][32 * kDensePitch];
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    uint32_t* const tile = tile_all[wave];
    // every column starts as the histogram of an empty sketch (estimate 0), as ertl_select_kernel fills its idle lanes: the columns
    // outside a row's range keep whatever valid histogram they held last, so all 64 lanes always run the estimator on real counts
#pragma unroll 8
    for (int w = 0; w < 32; ++w) tile[w * kDensePitch + lane] = w == 0 ? (1u << 14) : 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // a tile is private to its wave
    const int z0 = lo ? 0 : (pc_in->z0p1 ? pc_in->z0p1 - 1 : n_y);
    uint32_t* const my_word = tile + (bs_pidx(lane) + ((lane & 2) ? 16 : 0)) * kDensePitch;
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long k0 = ((long long)span_base + 8 * (j / n_tiles) + (u & 7)) * kDenseSpan;
        if (k0 >= n_y) continue;
        int r0, r1;
        rm.tile_rows((int)(j % n_tiles), kWavesPerBlock, &r0, &r1);
        const int i = r0 + wave;
        if (i >= r1) continue;                                               // wave-uniform; the kernel has no block barrier
        if (!lo && k0 + kDenseSpan <= (long long)i + 1) continue;             // the span lies under the diagonal
        const int k_lo = lo ? lo[i] : max(i + 1, z0), k_hi = lo ? hi[i] : min(hi[i], n_y - 1);
        const int kb = (int)max((long long)k_lo, k0), ke = (int)min((long long)k_hi + 1, k0 + kDenseSpan);
        if (kb >= ke) continue;
        {
            uint32_t xa[NB][8];
            bs_load<NB>(X.bs, i, lane, xa);
            const int gx = (int)X.gmax[i];
#pragma unroll 1
            for (int y = kb; y < ke; ++y) {
                uint32_t yb[NB][8];
                bs_load<NB>(Y.bs, y, lane, yb);
                const int kp = max(gx, (int)Y.gmax[y]) + 1;                  // values this pair can hold: [0, kp)
                const uint32_t tot = bs_pair_hist<NB>(xa, yb, kp, lane);
                my_word[y - (int)k0] = tot;                                  // (lanes 0, 1 and 2, 3 of a quad hold the same two bins: same word)
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int ky = (int)k0 + lane;
        const bool live = ky >= kb && ky < ke;
        const double t = dense_estimate<FMA>(tile + lane, relerr_scaled);
        const double e1 = (double)X.ecard[i], e2 = live ? (double)Y.ecard[ky] : 0.0;
        const double jacc = selhip::pair_value(MEAS, e1, e2, t);             // selection.cpp:287 (pair_value.hpp)
        const bool keep = live && jacc >= tau;                               // selection.cpp:288
        const u64 km = __ballot(keep);
        if (km) {
            u64 base = 0;
            if (lane == 0) base = atomicAdd(&pc->n_results, (u64)__popcll(km));
            base = ((u64)__builtin_amdgcn_readfirstlane((int)(base >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
            if (keep) {
                // (v_mbcnt: the selected lanes below this one, without a per-lane mask that would be kept in registers across the candidate loop)
                const u64 idx = base + (u64)__builtin_amdgcn_mbcnt_hi((uint32_t)(km >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)km, 0u));
                if (idx < results_cap) { results[idx].i = i; results[idx].k = ky; results[idx].jaccard = jacc; }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the next unit's stores come after these reads
    }
}

// ---- the list route's enumeration of a query pass ("dense_fused" = 0) -----------------------------------------------------------
// query_enum_windows_kernel: every (q, n_q + d) with d in q's window, in the combined index space of the query passes' stage 2 --
// one block per (query, stretch of kEnumSpan candidates), one atomic per block, like enum_pairs_kernel.  *count is exact even when
// the list is too small.
__global__ __launch_bounds__(kBlock)
void query_enum_windows_kernel(int n_q, const int* __restrict__ lo, const int* __restrict__ hi,
                               selhip_int2_t* __restrict__ out, u64 out_cap, u64* __restrict__ count) {
    __shared__ u64 base_lds;
    const int q = (int)(blockIdx.x % (unsigned)n_q), chunk = (int)(blockIdx.x / (unsigned)n_q);
    const long long k0 = (long long)lo[q] + (long long)chunk * kEnumSpan;
    const long long k_last = min((long long)hi[q], k0 + kEnumSpan - 1);
    const long long cnt = k_last - k0 + 1;
    if (cnt <= 0) return;                                                     // block-uniform
    if (threadIdx.x == 0) base_lds = atomicAdd(count, (u64)cnt);
    __syncthreads();
    const u64 base = base_lds;
    for (long long t = threadIdx.x; t < cnt; t += kBlock)
        if (base + (u64)t < out_cap) out[base + (u64)t] = selhip_int2_t{q, n_q + (int)(k0 + t)};
}

}  // namespace

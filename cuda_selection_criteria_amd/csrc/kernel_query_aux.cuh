// kernel_query_aux.cuh -- the auxiliary-HLL criteria of query passes (hll_a, hll_an, and the hll_a stage of hll_a + smh_a).
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace), after kernel_hll.cuh
// (LdsColumn, hist_add_word_packed, max_u8x4) and kernel_query.cuh.
//
// The test is that of aux_fused_kernel (src/selection.cpp:152-173 hll_a, :206-227 hll_an; criteria_sketch.hpp:22-64): U = Ertl-MLE of
// the union histogram of the two auxiliary sketches, then
//   CRIT 1 (hll_a):  t_hat = (size_t)U;  t+ = t_hat / (1 + Z*sigma_p);  K+ = ((1+gamma)*e_hi - t+)/t+ >= tau
//   CRIT 2 (hll_an): J = ((double)(e_lo+e_hi) - U)/U;  C = min(1, (1+Z*sigma_p)*e_hi/U) * (1+gamma) * S;  J + C >= tau
// with gamma = e_lo / e_hi.  The reference takes card_A <= card_B; the all-pairs pass gets that order from its rank order (i < k), a
// query pair (q, d) from e_lo = min and e_hi = max of the two truncated cards, whichever set each member comes from.  Every other term
// is symmetric, so the result is the cross pairs of the all-pairs pass over Q u D, ties included.
//   query_aux_window_kernel  hll_a / hll_an as the FIRST criterion: block = (one query) x (kBlock consecutive database ranks, one per
//                            lane) inside the query's CB window (query_windows_kernel) -- no pair list is built
//   query_aux_list_kernel    the two-stage criterion: the survivors (q, n_q + d) of the smh_a stage, one lane per pair
// Both append (q, n_q + d) -- the combined index space of stage 2 -- and count into pc->n_final.
#pragma once

namespace {

constexpr int kQueryAuxLdsMaxP = 12;            // window kernel: query rows up to 4 KiB are staged in LDS; larger ones are read from memory

template <bool FMA, int CRIT>
__device__ __forceinline__ bool query_aux_test(double U, u64 ea, u64 eb, double tau, double zs, double S_sum) {
    const u64 e_lo = ea < eb ? ea : eb, e_hi = ea < eb ? eb : ea;
    const double gamma = (double)e_lo / (double)e_hi;                        // criteria_sketch.hpp:24,38
    if constexpr (CRIT == 1) {
        const double t_hat = (double)(u64)(long long)U;                       // size_t t_hat = union_size()  (:61)
        const double t_mas = t_hat / (1.0 + zs);                              // :40
        const double K = selhip::muladd<FMA>(1.0 + gamma, (double)e_hi, -t_mas) / t_mas;   // :41
        return K >= tau;                                                      // :63
    } else {
        const double J = ((double)(e_lo + e_hi) - U) / U;                     // :55
        const double candv = (1.0 + zs) * (double)e_hi / U;                   // :32
        const double minimo = candv < 1.0 ? candv : 1.0;                      // std::min(1.0, .)
        const double C = minimo * (1 + gamma) * S_sum;                        // :33
        return (J + C) >= tau;                                                // :57
    }
}

// the lane's union histogram of rows ra, rb (n16 16-byte groups each) in its packed LDS column, then the estimate U.
// Every lane of the wave calls it with the same n16 (the loads are uniform in count).
template <bool FMA>
__device__ __forceinline__ double query_aux_union(uint32_t* __restrict__ col, const uint4* ra, const uint4* rb, int n16, int p_aux,
                                                  double relerr_scaled) {
#pragma unroll 8
    for (int k = 0; k < 32; ++k) col[k * kWave] = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int c0 = 0; c0 < n16; c0 += 8) {
        uint4 xa[8], xb[8];
#pragma unroll
        for (int t = 0; t < 8; ++t)
            if (c0 + t < n16) { xa[t] = ra[c0 + t]; xb[t] = rb[c0 + t]; }
#pragma unroll
        for (int t = 0; t < 8; ++t) {
            if (c0 + t < n16) {
                hist_add_word_packed(col, max_u8x4(xa[t].x, xb[t].x));
                hist_add_word_packed(col, max_u8x4(xa[t].y, xb[t].y));
                hist_add_word_packed(col, max_u8x4(xa[t].z, xb[t].z));
                hist_add_word_packed(col, max_u8x4(xa[t].w, xb[t].w));
            }
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    LdsColumn c{col};
    const double U = selhip::ertl_ml_estimate<FMA>(c, (unsigned)p_aux, (unsigned)(64 - p_aux), relerr_scaled);
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // (the column is zeroed again by the next pair)
    return U;
}

// ---------------------------------------------------------------------------------------------
// query_aux_window_kernel<FMA, CRIT, QLDS>: block (q, colb) covers database ranks [colb * kBlock, +kBlock) of query q; a block outside
// the window [lo_q, hi_q] leaves at once.  QLDS (p_aux <= kQueryAuxLdsMaxP): the query row is staged in LDS once per block and read
// with same-address broadcast loads; above that (8..32 KiB) every lane reads it from memory at one wave-uniform address (an L2 hit
// after the first wave).  A lane's database row is its own rank's: the 64 lanes of a wave read 64 consecutive rows, one contiguous
// run of memory.  LDS: 4 waves x 8 KiB of histogram columns + 4 KiB of query row + the append staging -- 40 KiB, four blocks per CU.
// ---------------------------------------------------------------------------------------------
template <bool FMA, int CRIT, bool QLDS>
__global__ __launch_bounds__(kBlock)
void query_aux_window_kernel(const uint8_t* __restrict__ aux_q, const uint8_t* __restrict__ aux_d, int p_aux, int n_q, int n_d,
                             const int* __restrict__ lo, const int* __restrict__ hi, int n_col_blocks, const u64* __restrict__ ecard,
                             double relerr_scaled, double tau, double zs, double S_sum,
                             selhip_int2_t* __restrict__ out, u64 out_cap, PassCounters* __restrict__ pc) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[kWavesPerBlock * 32 * kWave];    // [wave][bin pair][lane]
    __shared__ __attribute__((aligned(16))) uint4 qrow_lds[QLDS ? (1 << kQueryAuxLdsMaxP) / 16 : 1];
    __shared__ selhip_int2_t app_lds[kWavesPerBlock * kAppendCap];
    const int q = (int)blockIdx.x / n_col_blocks, colb = (int)blockIdx.x % n_col_blocks;
    const int l = lo[q], h = hi[q];
    const int k0 = colb * kBlock;
    if (h < l || k0 > h || k0 + kBlock - 1 < l) return;                        // block-uniform
    const long long nreg = 1ll << p_aux;
    const int n16 = (int)(nreg >> 4);                                          // 16-byte groups per row (p_aux >= 4)
    const uint4* const qrow_mem = reinterpret_cast<const uint4*>(aux_q + (long long)q * nreg);
    if constexpr (QLDS) {
        for (int t = threadIdx.x; t < n16; t += kBlock) qrow_lds[t] = qrow_mem[t];
        __syncthreads();
    }
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int k = k0 + (int)threadIdx.x;
    const bool live = k >= l && k <= h;                                        // (h < n_d)
    if (__ballot(live) == 0) return;                                           // wave-uniform; no barrier follows
    const int kc = live ? k : l;                                               // a valid row for the lanes outside the window
    const u64 ea = ecard[q], eb = ecard[n_q + kc];
    const uint4* const ra = QLDS ? qrow_lds : qrow_mem;
    const uint4* const rb = reinterpret_cast<const uint4*>(aux_d + (long long)kc * nreg);
    const double U = query_aux_union<FMA>(hist + wave * 32 * kWave + lane, ra, rb, n16, p_aux, relerr_scaled);
    const bool sel = live && query_aux_test<FMA, CRIT>(U, ea, eb, tau, zs, S_sum);
    WaveAppender app;
    app.init(app_lds, wave, out, out_cap, &pc->n_final);
    app.push(sel, q, n_q + k, lane);
    app.flush(lane);
}

// ---------------------------------------------------------------------------------------------
// query_aux_list_kernel<FMA, CRIT>: the list form (the auxiliary stage of hll_a + smh_a).  One lane per record (x, y) of the smh_a
// survivors: x < n_q is a query rank (row x of aux_q), y = n_q + d a database rank (row d of aux_d).  One-wave blocks, as
// aux_fused_kernel: the two rows differ from lane to lane, so there is nothing to share across waves.
// ---------------------------------------------------------------------------------------------
template <bool FMA, int CRIT>
__global__ __launch_bounds__(kWave)
void query_aux_list_kernel(const uint8_t* __restrict__ aux_q, const uint8_t* __restrict__ aux_d, int p_aux, int n_q,
                           const selhip_int2_t* __restrict__ pairs, const u64* __restrict__ n_dev, u64 cap, const u64* __restrict__ ecard,
                           double relerr_scaled, double tau, double zs, double S_sum,
                           selhip_int2_t* __restrict__ out, u64 out_cap, u64* __restrict__ out_count) {
    __shared__ __attribute__((aligned(16))) uint32_t hist[32 * kWave];     // [bin pair][lane], 8 KiB
    __shared__ selhip_int2_t app_lds[kAppendCap];
    const int lane = threadIdx.x;
    u64 n = *n_dev;
    if (n > cap) n = cap;
    const long long nreg = 1ll << p_aux;
    const int n16 = (int)(nreg >> 4);
    WaveAppender app;
    app.init(app_lds, 0, out, out_cap, out_count);
    for (u64 base = (u64)blockIdx.x * kWave; base < n; base += (u64)gridDim.x * kWave) {
        const u64 j = base + lane;
        const bool live = j < n;
        selhip_int2_t pr{0, n_q};                                              // (n_q >= 1 and n_d >= 1 here: valid rows)
        if (live) pr = pairs[j];
        const u64 ea = ecard[pr.x], eb = ecard[pr.y];
        const uint4* ra = reinterpret_cast<const uint4*>(aux_q + (long long)pr.x * nreg);
        const uint4* rb = reinterpret_cast<const uint4*>(aux_d + (long long)(pr.y - n_q) * nreg);
        const double U = query_aux_union<FMA>(hist + lane, ra, rb, n16, p_aux, relerr_scaled);
        const bool sel = live && query_aux_test<FMA, CRIT>(U, ea, eb, tau, zs, S_sum);
        app.push(sel, pr.x, pr.y, lane);
    }
    app.flush(lane);
}

}  // namespace

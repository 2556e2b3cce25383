// kernel_query.cuh -- query passes: a query set Q (ascending cardinality) against the context's database D (ascending cardinality).
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
//
// A pair (q, d) is selected iff e_hi != 0, [CB] cb_pred(tau, e_lo, e_hi), smh_a, J >= tau -- with e_lo / e_hi the smaller / larger of the
// two truncated cardinalities.  Every term is symmetric in q and d, so a query pass returns exactly the cross pairs of an all-pairs pass
// over Q u D (include/selection_hip.h section 2b).  The auxiliary-HLL criteria (hll_a, hll_an, hll_a + smh_a) are in kernel_query_aux.cuh.
// The kernels:
//   query_windows_kernel      one lane per query: e_q, the contiguous CB window [lo_q, hi_q] of D (two binary searches on the literal
//                             predicate), the evaluated-pair count; also the truncated cards of both sets in ONE index space [Q | D]
//   query_sig_join_kernel     SIG: a tile of queries' band signatures in LDS, one database genome per lane (band-major, coalesced)
//   query_verify_kernel       32-bit signatures, then the first flagged band on the full sketches (sig_candidate_ok, kernel_verify.cuh)
//   query_stream_kernel       STREAM: any band shape; a tile of query rows in LDS, database rows streamed coalesced, one row per wave
//   query_union_hist_kernel   stage 2a on the bit planes of Q and D (the pair-histogram code of kernel_hllbs.cuh with two base pointers)
// The survivor list carries (q, n_q + d) -- the combined index space -- so that the estimator / select kernel of the all-pairs path runs
// unchanged on it; query_result_fixup_kernel maps the selected records back to (q, d).
#pragma once

namespace {

constexpr int kQStreamRows = 128;               // database rows per block of the stream kernel
constexpr int kQStreamMaxQ = 8;                 // query rows per block of the stream kernel (LDS: at most 32 KiB of them)

// ---------------------------------------------------------------------------------------------
// query_windows_kernel.  P = first d with e_d > e_q.  On [0, P) the predicate is non-decreasing in d (e_lo = e_d grows, e_hi = e_q is
// fixed; e_q == 0 makes it false throughout), on [P, n_d) non-increasing (e_hi = e_d grows, e_lo = e_q is fixed).  So the window is
// [first true in [0, P), last true in [P, n_d)] -- contiguous, possibly empty.  Cards that are not ascending raise pc->unsorted.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ bool query_pair_pred(u64 e_q, u64 e_d, double tau, int use_cb) {
    const u64 e_lo = e_q < e_d ? e_q : e_d, e_hi = e_q < e_d ? e_d : e_q;
    if (e_hi == 0) return false;
    return !use_cb || cb_pred(tau, e_lo, e_hi);
}

// t = thread index over max(n_q, n_d); every lane of a wave calls it (the evaluated count is summed over the wave)
__device__ __forceinline__ void query_windows_body(int t, const double* __restrict__ cards_q, int n_q, const double* __restrict__ cards_d,
                                                   int n_d, double tau, int use_cb, u64* __restrict__ ecard, int* __restrict__ lo,
                                                   int* __restrict__ hi, PassCounters* __restrict__ pc) {
    if (t < n_d) {
        const double c = cards_d[t];
        ecard[n_q + t] = selhip::trunc_card(c);
        if (t > 0 && c < cards_d[t - 1]) pc->unsorted = 1;
    }
    u64 cnt = 0;
    if (t < n_q) {
        const double c = cards_q[t];
        if (t > 0 && c < cards_q[t - 1]) pc->unsorted = 1;
        const u64 e_q = selhip::trunc_card(c);
        ecard[t] = e_q;
        // lo = first d with (e_d > e_q || pred): false...true on [0, n_d) -- the first true of the predicate below P, else P;
        // h + 1 = first d with (e_d > e_q && !pred): the first false of the predicate from P on.  Both searches advance together (two
        // independent loads per step instead of three dependent chains).
        int a1 = 0, b1 = n_d, a2 = 0, b2 = n_d;
        while (a1 < b1 || a2 < b2) {
            const int m1 = a1 + (b1 - a1) / 2, m2 = a2 + (b2 - a2) / 2;
            const u64 e1 = selhip::trunc_card(cards_d[min(m1, n_d - 1)]), e2 = selhip::trunc_card(cards_d[min(m2, n_d - 1)]);
            if (a1 < b1) { if (e1 > e_q || query_pair_pred(e_q, e1, tau, use_cb)) b1 = m1; else a1 = m1 + 1; }
            if (a2 < b2) { if (e2 > e_q && !query_pair_pred(e_q, e2, tau, use_cb)) b2 = m2; else a2 = m2 + 1; }
        }
        const int l = a1, h = a2 - 1;
        lo[t] = l; hi[t] = h;
        if (h >= l) cnt = (u64)(h - l + 1);
    }
    // one atomic per wave (a single address sustains ~90 returning atomics per microsecond)
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) cnt += __shfl_xor(cnt, s, kWave);
    if ((threadIdx.x & (kWave - 1)) == 0 && cnt) atomicAdd(&pc->n_evaluated, cnt);
}

// the counters of the NEXT query pass (the other of two sets) are cleared by the first kernel of this one -- no memset dispatch
__device__ __forceinline__ void query_zero_next(PassCounters* __restrict__ zero_pc) {
    if (blockIdx.x == 0 && threadIdx.x < sizeof(PassCounters) / 8) reinterpret_cast<u64*>(zero_pc)[threadIdx.x] = 0;
}

__global__ __launch_bounds__(kBlock)
void query_windows_kernel(const double* __restrict__ cards_q, int n_q, const double* __restrict__ cards_d, int n_d, double tau, int use_cb,
                          u64* __restrict__ ecard, int* __restrict__ lo, int* __restrict__ hi, PassCounters* __restrict__ pc,
                          PassCounters* __restrict__ zero_pc) {
    query_zero_next(zero_pc);
    query_windows_body((int)(blockIdx.x * blockDim.x + threadIdx.x), cards_q, n_q, cards_d, n_d, tau, use_cb, ecard, lo, hi, pc);
}

// SIG passes: the windows ride in the first win_blocks blocks of the queries' signature build (sig_build_body / sig_build_tile_body of
// kernel_sigjoin.cuh), the way the all-pairs pass carries its bounds in sig_build_kernel: the two latency-bound steps overlap
__global__ __launch_bounds__(kBlock)
void query_prep_sig_kernel(int win_blocks, const double* __restrict__ cards_q, int n_q, const double* __restrict__ cards_d, int n_d, double tau,
                           int use_cb, u64* __restrict__ ecard, int* __restrict__ lo, int* __restrict__ hi, PassCounters* __restrict__ pc,
                           PassCounters* __restrict__ zero_pc,
                           const u64* __restrict__ aux_q, int m, int r, int nb, int n_pad, uint32_t* __restrict__ sigQ, uint32_t* __restrict__ sigT,
                           uint32_t* __restrict__ sigP, uint32_t* __restrict__ sigG, int tile_mode) {
    if ((int)blockIdx.x < win_blocks) {
        query_zero_next(zero_pc);
        query_windows_body((int)(blockIdx.x * blockDim.x + threadIdx.x), cards_q, n_q, cards_d, n_d, tau, use_cb, ecard, lo, hi, pc);
        return;
    }
    if (tile_mode) sig_build_tile_body<kSigTileG>((int)blockIdx.x - win_blocks, aux_q, n_q, m, r, nb, n_pad, sigQ, sigT, sigP, sigG, 16, tile_mode);
    else           sig_build_body((long long)blockIdx.x - win_blocks, aux_q, n_q, m, r, nb, n_pad, sigQ, sigT, sigP, sigG, 16);
}

// ---------------------------------------------------------------------------------------------
// query_sig_join_kernel<QT>: block = (tile of QT consecutive queries) x (kBlock consecutive database genomes, one per lane).
// The tile's 32-bit band signatures sit in LDS band-major ([band][query]), so that one broadcast ds_read_b128 hands every lane four
// queries' band signatures; the lane's database signature of that band comes from the band-major array (one coalesced 256-byte load
// per wave).  Per band and query: v_xor + v_min into the query's accumulator (0 = some band signature equal).  A block whose database
// range misses the union of its queries' windows leaves after one barrier; inside it, a lane tests its own query's window before it
// appends.  Measured on W1: the 16-bit signatures packed two per dword (v_xor + v_pk_min_u16, half the
// instructions per band, its extra matches cut back by the verification) took 0.295 ms against 0.195 ms for this form; a tile of
// 64 queries 0.28 ms.
// ---------------------------------------------------------------------------------------------
template <int QT>
__global__ __launch_bounds__(kBlock)
void query_sig_join_kernel(const uint32_t* __restrict__ sig_q, const uint32_t* __restrict__ sigT_d, int n_q, int n_d, int n_pad, int nb,
                           const int* __restrict__ lo, const int* __restrict__ hi, int n_col_blocks,
                           selhip_int2_t* __restrict__ cand, u64 cand_cap, PassCounters* __restrict__ pc) {
    static_assert(QT % 4 == 0 && QT <= kWave, "tile of 4k <= 64 queries");
    __shared__ __attribute__((aligned(16))) uint32_t qs[128 * QT];
    __shared__ int s_lo[QT], s_hi[QT], s_rng[2];
    __shared__ selhip_int2_t app_lds[kWavesPerBlock * kAppendCap];
    const int tile = (int)blockIdx.x / n_col_blocks, colb = (int)blockIdx.x % n_col_blocks;
    const int q0 = tile * QT;
    const int nq = min(QT, n_q - q0);
    if (threadIdx.x < kWave) {
        // wave 0: the tile's windows and their union (lanes >= nq hold an empty window)
        int l = 0x7FFFFFFF, h = -1;
        if ((int)threadIdx.x < nq) { l = lo[q0 + threadIdx.x]; h = hi[q0 + threadIdx.x]; }
        if (threadIdx.x < QT) { s_lo[threadIdx.x] = l; s_hi[threadIdx.x] = h; }
        int rl = h >= l ? l : 0x7FFFFFFF, rh = h >= l ? h : -1;
#pragma unroll
        for (int sft = 32; sft > 0; sft >>= 1) { rl = min(rl, __shfl_xor(rl, sft, kWave)); rh = max(rh, __shfl_xor(rh, sft, kWave)); }
        if (threadIdx.x == 0) { s_rng[0] = rl; s_rng[1] = rh; }
    }
    __syncthreads();
    const int r_lo = s_rng[0], r_hi = s_rng[1];
    const int k0 = colb * kBlock;
    if (k0 > r_hi || k0 + kBlock - 1 < r_lo) return;                    // block-uniform
    for (int t = threadIdx.x; t < QT * nb; t += kBlock) {
        const int a = t / nb, b = t - a * nb;
        qs[b * QT + a] = a < nq ? sig_q[(size_t)(q0 + a) * nb + b] : 0u;
    }
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int k = k0 + (int)threadIdx.x;
    const bool live = k < n_d && k >= r_lo && k <= r_hi;
    if (__ballot(live) == 0) return;                                     // wave-uniform; no barrier follows
    const int kc = live ? k : r_lo;                                      // (r_lo <= r_hi < n_d: a valid column)
    uint32_t acc[QT];
#pragma unroll
    for (int a = 0; a < QT; ++a) acc[a] = ~0u;
#pragma unroll 4
    for (int b = 0; b < nb; ++b) {
        const uint32_t s = sigT_d[(size_t)b * n_pad + kc];
        const uint4* qb = reinterpret_cast<const uint4*>(qs + b * QT);
#pragma unroll
        for (int a4 = 0; a4 < QT / 4; ++a4) {
            const uint4 v = qb[a4];
            acc[4 * a4 + 0] = min(acc[4 * a4 + 0], s ^ v.x);
            acc[4 * a4 + 1] = min(acc[4 * a4 + 1], s ^ v.y);
            acc[4 * a4 + 2] = min(acc[4 * a4 + 2], s ^ v.z);
            acc[4 * a4 + 3] = min(acc[4 * a4 + 3], s ^ v.w);
        }
    }
    WaveAppender app;
    app.init(app_lds, wave, cand, cand_cap, &pc->n_pre);
#pragma unroll
    for (int a = 0; a < QT; ++a)
        app.push(live && acc[a] == 0u && k >= s_lo[a] && k <= s_hi[a], q0 + a, k, lane);
    app.flush(lane);
}

// query_verify_kernel: one lane per match (q, d) of the join (its list counted in n_pre).  (1) The two genomes' 32-bit signature rows
// (genome-major sigQ, 16-byte loads) give the first band with an equal signature; the pairs that have one are the candidate set,
// counted in n_candidates.  (2) That band is compared on the full sketches and sig_candidate_ok (kernel_verify.cuh) decides on Q's
// and D's rows.  (Against the literal check alone, which walks the bands from the first: W1 verification 31 -> 29 us, W2 135 -> 15 us.)
// Survivors are appended as (q, n_q + d), the combined index space of stage 2.
__global__ __launch_bounds__(kBlock)
void query_verify_kernel(const u64* __restrict__ aux_q, const u64* __restrict__ aux_d, int m, int n_rows, int n_bands, int n_q,
                         const uint32_t* __restrict__ sig_q, const uint32_t* __restrict__ sig_d,
                         const selhip_int2_t* __restrict__ cand, const u64* __restrict__ n_cand_dev, u64 cand_cap,
                         selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc) {
    __shared__ selhip_int2_t app_lds[kWavesPerBlock * kAppendCap];
    __shared__ uint32_t blk_cand;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    if (threadIdx.x == 0) blk_cand = 0;
    __syncthreads();
    u64 n = *n_cand_dev;
    if (n > cand_cap) n = cand_cap;
    WaveAppender app;
    app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
    uint32_t n_c = 0;
    for (u64 base = (u64)blockIdx.x * kBlock; base < n; base += (u64)gridDim.x * kBlock) {      // block-uniform trip count
        const u64 j = base + threadIdx.x;
        selhip_int2_t pr{0, 0};
        bool ok = false;
        if (j < n) {
            pr = cand[j];
            const uint4* a = reinterpret_cast<const uint4*>(sig_q + (size_t)pr.x * n_bands);
            const uint4* b = reinterpret_cast<const uint4*>(sig_d + (size_t)pr.y * n_bands);
            int first = n_bands;
            for (int g = n_bands / 4 - 1; g >= 0; --g) {                   // n_bands is a multiple of 8 here
                const uint4 u = a[g], v = b[g];
                if (u.w == v.w) first = 4 * g + 3;
                if (u.z == v.z) first = 4 * g + 2;
                if (u.y == v.y) first = 4 * g + 1;
                if (u.x == v.x) first = 4 * g;
            }
            if (first < n_bands) {
                n_c += 1;
                const u64* x = aux_q + (size_t)pr.x * m + (size_t)first * n_rows;
                const u64* y = aux_d + (size_t)pr.y * m + (size_t)first * n_rows;
                int t = 0;
                while (t < n_rows && x[t] == y[t]) ++t;
                ok = sig_candidate_ok(t == n_rows, 0, aux_q + (size_t)pr.x * m, aux_d + (size_t)pr.y * m, n_rows, n_bands);
            }
        }
        app.push(ok, pr.x, n_q + pr.y, lane);
    }
    app.flush(lane);
#pragma unroll
    for (int sft = 32; sft > 0; sft >>= 1) n_c += __shfl_xor(n_c, sft, kWave);
    if (lane == 0 && n_c) atomicAdd(&blk_cand, n_c);
    __syncthreads();
    if (threadIdx.x == 0 && blk_cand) atomicAdd(&pc->n_candidates, (u64)blk_cand);     // one atomic per block
}

// ---------------------------------------------------------------------------------------------
// query_stream_kernel: STREAM for any (n_rows, n_bands) with n_rows * n_bands = m.  Block = (tile of qt <= 8 query rows staged in LDS) x
// (kQStreamRows database rows); a wave takes one database row at a time and reads it 64 buckets per load (lane = bucket, 512 contiguous
// bytes per wave instruction).  For each query of the tile whose window holds the row, the 64 bucket compares of a load become one
// v_cmp_eq_u64 lane mask; the scalar unit walks the mask's UNEQUAL buckets in order: with `next` = the first band not yet known to
// hold an unequal bucket, an unequal bucket in a band beyond `next` proves band `next` entirely equal (every one of its buckets lies
// before this one).  At the end of the row, some band is entirely equal iff next < n_bands.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock)
void query_stream_kernel(const u64* __restrict__ aux_q, const u64* __restrict__ aux_d, int n_q, int n_d, int m, int n_rows, int n_bands,
                         int qt, const int* __restrict__ lo, const int* __restrict__ hi, int n_col_blocks,
                         selhip_int2_t* __restrict__ surv, u64 surv_cap, PassCounters* __restrict__ pc) {
    extern __shared__ u64 qrows[];                                       // [qt][m]
    __shared__ selhip_int2_t app_lds[kWavesPerBlock * kAppendCap];
    const int tile = (int)blockIdx.x / n_col_blocks, colb = (int)blockIdx.x % n_col_blocks;
    const int q0 = tile * qt;
    const int nq = min(qt, n_q - q0);
    int qlo[kQStreamMaxQ], qhi[kQStreamMaxQ];
    int r_lo = 0x7FFFFFFF, r_hi = -1;
#pragma unroll
    for (int a = 0; a < kQStreamMaxQ; ++a) {
        qlo[a] = 0; qhi[a] = -1;
        if (a < nq) { qlo[a] = lo[q0 + a]; qhi[a] = hi[q0 + a]; }        // uniform loads
        if (qhi[a] >= qlo[a]) { r_lo = min(r_lo, qlo[a]); r_hi = max(r_hi, qhi[a]); }
    }
    const int k_begin = max(colb * kQStreamRows, r_lo), k_end = min(min(colb * kQStreamRows + kQStreamRows, n_d), r_hi + 1);
    if (k_begin >= k_end) return;                                        // block-uniform
    for (int t = threadIdx.x; t < nq * m; t += kBlock) qrows[t] = aux_q[(size_t)q0 * m + t];
    __syncthreads();
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int n_seg = (m + kWave - 1) / kWave;
    const bool r_pow2 = (n_rows & (n_rows - 1)) == 0;
    const int lr = __builtin_ctz((unsigned)n_rows);
    WaveAppender app;
    app.init(app_lds, wave, surv, surv_cap, &pc->n_survivors);
    for (int k = k_begin + wave; k < k_end; k += kWavesPerBlock) {
        int next[kQStreamMaxQ];
        bool live[kQStreamMaxQ], hit[kQStreamMaxQ];
        bool any = false;
#pragma unroll
        for (int a = 0; a < kQStreamMaxQ; ++a) {
            live[a] = a < nq && k >= qlo[a] && k <= qhi[a];
            hit[a] = false; next[a] = 0;
            any |= live[a];
        }
        if (!any) continue;
        const u64* row = aux_d + (size_t)k * m;
        for (int s = 0; s < n_seg; ++s) {
            const int t = s * kWave + lane;
            const u64 v = t < m ? row[t] : 0ull;
#pragma unroll
            for (int a = 0; a < kQStreamMaxQ; ++a) {
                if (!live[a] || hit[a]) continue;                         // uniform
                const bool eq = t < m && v == qrows[a * m + t];
                u64 U = ~__ballot(eq);
                if (s == n_seg - 1 && (m & (kWave - 1))) U &= (1ull << (m & (kWave - 1))) - 1ull;   // buckets past m belong to no band
                int nx = next[a];
                while (U) {
                    const int tb = s * kWave + (int)__builtin_ctzll(U);
                    const int band = r_pow2 ? (tb >> lr) : tb / n_rows;
                    if (band > nx) { hit[a] = true; break; }
                    nx = band + 1;
                    const int stop = nx * n_rows - s * kWave;              // first bucket of the next band, relative to this load
                    U = stop >= kWave ? 0ull : (U & (~0ull << stop));
                }
                next[a] = nx;
            }
        }
#pragma unroll
        for (int a = 0; a < kQStreamMaxQ; ++a)
            if (live[a] && (hit[a] || next[a] < n_bands)) app.push_uniform(q0 + a, n_q + k, lane);
    }
    app.flush(lane);
}

// ---------------------------------------------------------------------------------------------
// query_union_hist_kernel<NB>: the union histogram of every survivor (q, n_q + d) from the bit planes of Q (bs_q) and of D (bs_d) --
// bs_load / bs_pair_hist of kernel_hllbs.cuh, one wave per pair, counts indexed from the window start [off, off + len) like
// hll_union_hist_bs_kernel.  Lists here are short (survivors of n_q rows), so a plain grid-stride walk.
// ---------------------------------------------------------------------------------------------
template <int NB>
__global__ __launch_bounds__(kBlock, NB <= 5 ? 4 : 2)
void query_union_hist_kernel(const uint32_t* __restrict__ bs_q, const uint8_t* __restrict__ gmax_q,
                             const uint32_t* __restrict__ bs_d, const uint8_t* __restrict__ gmax_d, int n_q,
                             const selhip_int2_t* __restrict__ pairs, const u64* __restrict__ n_dev, u64 cap,
                             uint32_t* __restrict__ counts, u64 off, u64 len) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    u64 n = *n_dev;
    if (n > cap) n = cap;
    n = n > off ? min(n - off, len) : 0;
    pairs += off;
    const int my_bin = ((lane & 2) ? 32 : 0) + 2 * bs_pidx(lane) + (lane & 1);
    for (u64 j = (u64)blockIdx.x * kWavesPerBlock + wave; j < n; j += (u64)gridDim.x * kWavesPerBlock) {
        const selhip_int2_t pr = pairs[j];
        const int x = __builtin_amdgcn_readfirstlane(pr.x), y = __builtin_amdgcn_readfirstlane(pr.y) - n_q;
        uint32_t xa[NB][8], yb[NB][8];
        bs_load<NB>(bs_q, x, lane, xa);
        bs_load<NB>(bs_d, y, lane, yb);
        const int kp = max((int)gmax_q[x], (int)gmax_d[y]) + 1;
        const uint32_t tot = bs_pair_hist<NB>(xa, yb, kp, lane);
        counts[j * 64 + my_bin] = (lane & 1) ? (tot >> 16) : (tot & 0xFFFFu);
    }
}

// the selected records of the combined index space back to database ranks
__global__ __launch_bounds__(kBlock)
void query_result_fixup_kernel(selhip_pair_t* __restrict__ res, const u64* __restrict__ n_dev, u64 cap, int n_q) {
    u64 n = *n_dev;
    if (n > cap) n = cap;
    for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < n; j += (u64)gridDim.x * kBlock) res[j].k -= n_q;
}

}  // namespace

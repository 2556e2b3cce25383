// kernel_matrix_smh.cuh -- the SuperMinHash measures of the dense matrices: the cell of (a, b) is c = #{ j < m : aux_a[j] == aux_b[j] }
// (SELHIP_MEASURE_SMH_MATCHES) or (double)c / (double)m (SELHIP_MEASURE_SMH_JACCARD), compared on the full 64-bit buckets
// (selhip_ctx_matrix / selhip_ctx_query_matrix, abi_matrix.inc).
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace), behind kernel_matrix.cuh
// (MatrixOut) and host_plan.hpp (units, slab and mirror rules).  Both kernels read `aux` row-major, as uploaded or attached.
//   matrix_smh_kernel<NCH, OutT>   m = 128 * NCH buckets, NCH in {1, 2, 4, 8} (the fast path, matrix_smh_fast; upload and attach guarantee 16-byte aligned rows)
//     * unit = a tile of 4 * Q rows (Q = matrix_smh_q(NCH) per wave: 12, 12, 6, 3) x a span of 64 consecutive columns, the spans dealt to the XCD
//       slots as in matrix_kernel; a wave keeps its Q rows in VGPRs -- load c of a row hands lane l the buckets 128 c + 2 l, + 1, straight
//       from the coalesced 16-byte loads: for a count the map does not matter as long as both rows of a pair use the same one;
//     * the wave streams the span's <= 64 candidate rows past them, kStreamAhead rows in flight ahead (the ring of smh_stream_kernel);
//       per (query, candidate): 2 NCH v_cmp_eq_u64 into SGPR pairs, one s_bcnt1_i32_b64 each, scalar adds, and ONE v_writelane_b32 that
//       puts the count into lane (column - span start) of that query's output register;
//     * the tail: per query row one typed store of 64 consecutive columns -- no ballot result kept, no counter, no atomic, no LDS.
//   matrix_smh_generic_kernel<OutT>   every other m > 0: matrix_kernel's unit (one row per wave x 64 columns), lane = column, a serial loop
//     over the m buckets.  The same numbers; for small m, where a row is less than one wave load, and for m outside the fast path's set.
// A self matrix follows matrix_computes / matrix_skips_span / matrix_mirrors.  The fast path skips a span that lies under the diagonal of
// the wave's FIRST row (hence of all its rows) and otherwise compares the whole span, storing only the cells each row computes; the
// count is symmetric by definition, so the mirror is a saving, not a definition.  MatrixOut.self = 0 computes the whole rectangle.
#pragma once

// v_writelane_b32: `old` with lane `lane_idx` (wave-uniform) replaced by the wave-uniform `value`; the compiler keeps the lane select in
// M0, as the instruction wants on gfx9.  Where clang offers the builtin it is used.  The hipcc of ROCm 7.2.0 (clang 22) does not, so
// there the LLVM intrinsic is declared under its own overloaded name (checked on that version; a compiler that spells the intrinsic
// differently fails at link time with the name in the message, and newer ones take the builtin).  The declaration stands outside the
// anonymous namespace: the name is the intrinsic's, there is nothing to define.
#if defined(__has_builtin) && __has_builtin(__builtin_amdgcn_writelane)
#define matrix_smh_writelane(value, lane_idx, old) __builtin_amdgcn_writelane((value), (lane_idx), (old))
#else
__device__ int matrix_smh_writelane(int value, int lane_idx, int old) __asm("llvm.amdgcn.writelane.i32");
#endif

namespace {

constexpr bool matrix_smh_fast(int m) { return m == 128 || m == 256 || m == 512 || m == 1024; }
// rows a wave of the fast path keeps in VGPRs: the stream kernel's budget of query registers, at most 12 rows (24 rows at m = 128 gave
// the compiler more counts in flight than it has SGPRs: 28 spilled)
constexpr int matrix_smh_q(int nch) { return kQueryVgprBudget / nch < 12 ? kQueryVgprBudget / nch : 12; }
constexpr int matrix_smh_tile_rows(int m) { return kWavesPerBlock * matrix_smh_q(m / 128); }               // fast path: rows of a unit

template <typename OutT>
__device__ __forceinline__ void matrix_smh_store(const MatrixOut& o, OutT* out, int r0, int r1, int i, int ky, bool in_span, double v) {
    if (!in_span || (o.self && !matrix_computes(r0, i, ky))) return;
    const size_t pos_r = (size_t)(o.row_pos ? o.row_pos[i - r0] : i - r0), pos_c = (size_t)(o.col_pos ? o.col_pos[ky] : ky);
    out[pos_r * (size_t)o.ld + pos_c] = (OutT)v;
    if (o.self && o.mirror && matrix_mirrors(i, ky, r1)) {
        const size_t m_r = (size_t)(o.row_pos ? o.row_pos[ky - r0] : ky - r0), m_c = (size_t)(o.col_pos ? o.col_pos[i] : i);
        out[m_r * (size_t)o.ld + m_c] = (OutT)v;
    }
}

template <int NCH, typename OutT>
__global__ __launch_bounds__(kBlock, (NCH <= 4 ? 3 : 2))
void matrix_smh_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int r0, int r1, int n_y, int n_tiles, long long n_units, MatrixOut o) {
    constexpr int Q = matrix_smh_q(NCH);
    constexpr int ROWV = NCH * kWave;                  // u64x2 per sketch row
    constexpr int AHEAD = NCH <= 4 ? kStreamAhead : 1;
    constexpr int RING = AHEAD + 1;
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const double m_f = (double)(128 * NCH);
    OutT* const out = static_cast<OutT*>(o.out);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long k0l = (8 * (j / n_tiles) + (u & 7)) * kMatrixSpan;
        if (k0l >= n_y) continue;
        const long long i0l = (long long)r0 + ((j % n_tiles) * kWavesPerBlock + wave) * Q;
        if (i0l >= r1) continue;                                             // wave-uniform; the kernel has no block barrier
        const int i0 = (int)i0l, k0 = (int)k0l;
        if (o.self && matrix_skips_span(r0, i0, k0l)) continue;              // under the diagonal of row i0, so of every row of the wave
        const int ke = (int)min((long long)n_y, k0l + kMatrixSpan);
        u64x2 q[Q][NCH];
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const u64x2* row = X + (long long)min(i0 + a, r1 - 1) * ROWV + lane;     // rows past the slab: a valid row, never stored
#pragma unroll
            for (int c = 0; c < NCH; ++c) q[a][c] = row[c * kWave];
        }
        int acc[Q];
#pragma unroll
        for (int a = 0; a < Q; ++a) acc[a] = 0;
        u64x2 ring[RING][NCH];
        auto load_row = [&](u64x2 (&dst)[NCH], int kk) {
            const u64x2* row = Y + (long long)min(kk, ke - 1) * ROWV + lane;         // clamped: prefetches past the span re-read a valid row
#pragma unroll
            for (int c = 0; c < NCH; ++c) dst[c] = row[c * kWave];
        };
        auto compare_row = [&](const u64x2 (&cand)[NCH], int kk) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                int cnt = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c)
                    cnt += __popcll(__ballot(cand[c].x == q[a][c].x)) + __popcll(__ballot(cand[c].y == q[a][c].y));
                acc[a] = matrix_smh_writelane(cnt, kk - k0, acc[a]);
            }
        };
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) load_row(ring[s], k0 + s);
        for (int k = k0; k < ke; k += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                const int kk = k + s;
                if (kk >= ke) break;
                load_row(ring[(s + AHEAD) % RING], kk + AHEAD);
                compare_row(ring[s], kk);
            }
        }
        const int ky = k0 + lane;
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const int i = i0 + a;
            if (i >= r1) break;
            const double cnt = (double)acc[a];
            matrix_smh_store<OutT>(o, out, r0, r1, i, ky, ky < ke, o.measure == SELHIP_MEASURE_SMH_JACCARD ? cnt / m_f : cnt);
        }
    }
}

template <typename OutT>
__global__ __launch_bounds__(kBlock)
void matrix_smh_generic_kernel(const u64* __restrict__ X, const u64* __restrict__ Y, int m, int r0, int r1, int n_y, int n_tiles, long long n_units, MatrixOut o) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    OutT* const out = static_cast<OutT*>(o.out);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long k0 = (8 * (j / n_tiles) + (u & 7)) * kMatrixSpan;
        if (k0 >= n_y) continue;
        const long long row = (long long)r0 + (j % n_tiles) * kWavesPerBlock + wave;
        if (row >= r1) continue;
        const int i = (int)row;
        if (o.self && matrix_skips_span(r0, i, k0)) continue;
        const int ky = (int)k0 + lane;
        const bool in_span = ky < n_y;
        const u64* const x = X + (long long)i * m;
        const u64* const y = Y + (long long)min(ky, n_y - 1) * m;            // lanes past the end: a valid row, never stored
        int cnt = 0;
        for (int b = 0; b < m; ++b) cnt += x[b] == y[b] ? 1 : 0;
        const double c = (double)cnt;
        matrix_smh_store<OutT>(o, out, r0, r1, i, ky, in_span, o.measure == SELHIP_MEASURE_SMH_JACCARD ? c / (double)m : c);
    }
}

}  // namespace

// kernel_matrix_smh.cuh -- the SuperMinHash measures of the dense matrices: the cell of (a, b) is c = #{ j < m : aux_a[j] == aux_b[j] }
// (SELHIP_MEASURE_SMH_MATCHES) or (double)c / (double)m (SELHIP_MEASURE_SMH_JACCARD), compared on the full 64-bit buckets
// (selhip_ctx_matrix / selhip_ctx_query_matrix, abi_matrix.inc).
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace), behind kernel_matrix.cuh
// (MatrixOut) and host_plan.hpp (units, slab and mirror rules).  Every kernel reads `aux` row-major, as uploaded or attached.
//   matrix_smh_kernel<NCH, OutT>   m = 128 * NCH buckets, NCH in {1, 2, 4, 8} (the fast path, matrix_smh_fast; upload and attach guarantee 16-byte aligned rows)
//     * unit = a tile of 4 * Q rows (Q = matrix_smh_q(NCH) per wave: 12, 12, 6, 3) x a span of 64 consecutive columns, the spans dealt to the XCD
//       slots as in matrix_kernel; a wave keeps its Q rows in VGPRs -- load c of a row hands lane l the buckets 128 c + 2 l, + 1, straight
//       from the coalesced 16-byte loads: for a count the map does not matter as long as both rows of a pair use the same one;
//     * the wave streams the span's <= 64 candidate rows past them, kStreamAhead rows in flight ahead (the ring of smh_stream_kernel);
//       per (query, candidate): 2 NCH v_cmp_eq_u64 into SGPR pairs, one s_bcnt1_i32_b64 each, scalar adds, and ONE v_writelane_b32 that
//       puts the count into lane (column - span start) of that query's output register;
//     * the tail: per query row one typed store of 64 consecutive columns -- no ballot result kept, no counter, no atomic, no LDS.
//   matrix_smh_narrow_kernel<G, OutT>   m = 128 / G buckets, G in {2, 4}: a row is 1 / G of a wave load
//     * the same unit with Q = 12 rows per wave, ONE u64x2 each: lane l holds buckets 2 (l % (64 / G)), + 1 of the row, so every one of
//       the G lane groups holds the whole query row;
//     * a wave load is G CONSECUTIVE candidate rows (1 KiB in a row of the array, one row per lane group), the span <= 64 / G loads through
//       the same ring; per (query, load) two v_cmp_eq_u64 whose ballots hold G fields of 64 / G bits: matrix_smh_narrow_counts splits them
//       on the scalar unit (s_bcnt1_i32_b32 on the halves; for G = 4 behind s_pack_ll / s_pack_hh of the x and y fields) and G
//       v_writelane_b32 place the counts.  A lane group past the span re-reads row ke - 1; its count lands in a lane that is never stored.
//   matrix_smh_wide_kernel<OutT>   m = 1024 C buckets, C = 2 .. 8: the buckets are split, not the rows
//     * the unit of matrix_smh_kernel<8> (Q = 3 rows per wave); the wave walks the row in C chunks of 1 024 buckets: per chunk the Q query
//       chunks in VGPRs, the span's candidate chunks streamed past them (matrix_smh_chunk_count), each count added to the cell's running
//       total -- v_readlane_b32, a scalar add, v_writelane_b32; the totals stay in the Q output registers: no LDS, no atomic, one launch;
//     * the (chunk, candidate) steps are ONE stream through the ring: the first candidate chunk of chunk c + 1 is in flight while the last
//       of chunk c is compared.
//   matrix_smh_generic_kernel<OutT>   every other m > 0: matrix_kernel's unit (one row per wave x 64 columns), lane = column, a serial loop
//     over the m buckets.  The same numbers; for m outside the sets above, rows off the 16-byte grid, and under "matrix_smh_generic".
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
// which kernel a matrix of m buckets takes ("matrix_smh_kernel_used"): the register tile where matrix_smh_fast; rows of less than one
// wave load, m = 32 and 64, the narrow kernel; every multiple of 1024 from 2048 to 8192 the wide one; every other m the generic one
enum { kMatrixSmhGeneric = 0, kMatrixSmhTile = 1, kMatrixSmhNarrow = 2, kMatrixSmhWide = 3 };
constexpr int matrix_smh_kind(int m) {
    return matrix_smh_fast(m) ? kMatrixSmhTile : m == 32 || m == 64 ? kMatrixSmhNarrow : m >= 2048 && m <= 8192 && m % 1024 == 0 ? kMatrixSmhWide : kMatrixSmhGeneric;
}
constexpr int kMatrixSmhNarrowQ = 12;              // rows a wave of the narrow kernel keeps in VGPRs (one u64x2 each), the tile kernel's most
constexpr int kMatrixSmhWideNch = 8;               // wave loads per chunk of the wide kernel: 1 024 buckets, the tile kernel's widest row
// rows of a unit of that kernel: four waves of Q rows each (the generic kernel: of one)
constexpr int matrix_smh_unit_rows(int m) {
    const int kind = matrix_smh_kind(m);
    return kind == kMatrixSmhTile ? matrix_smh_tile_rows(m) : kind == kMatrixSmhNarrow ? kWavesPerBlock * kMatrixSmhNarrowQ
         : kind == kMatrixSmhWide ? kWavesPerBlock * matrix_smh_q(kMatrixSmhWideNch) : kWavesPerBlock;
}

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

// ---- narrow rows: m = 32 and m = 64 -----------------------------------------------------------------------------------------------
// the G counts of one query row, replicated over the G lane groups of `q`, against the G candidate rows of one wave load: two
// v_cmp_eq_u64, each ballot holding G fields of 64 / G bits, split on the scalar unit -- the halves for G = 2; for G = 4 the x and
// the y field of a row are first put side by side in one dword, so that a row still costs one s_bcnt1_i32_b32
template <int G>
__device__ __forceinline__ void matrix_smh_narrow_counts(const u64x2& q, const u64x2& cand, int (&cnt)[G]) {
    static_assert(G == 2 || G == 4, "a row of 64 or of 32 buckets");
    const u64 bx = __ballot(cand.x == q.x), by = __ballot(cand.y == q.y);
    const uint32_t xl = (uint32_t)bx, xh = (uint32_t)(bx >> 32), yl = (uint32_t)by, yh = (uint32_t)(by >> 32);
    if constexpr (G == 2) {
        cnt[0] = __popc(xl) + __popc(yl);
        cnt[1] = __popc(xh) + __popc(yh);
    } else {
        // (written as two-halfword vectors so that the compiler takes s_pack_ll_b32_b16 / s_pack_hh_b32_b16 for them)
        typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
        auto pair_count = [](uint32_t x, uint32_t y) { const u16x2 v = {(unsigned short)x, (unsigned short)y}; return __popc(__builtin_bit_cast(uint32_t, v)); };
        cnt[0] = pair_count(xl, yl);
        cnt[1] = pair_count(xl >> 16, yl >> 16);
        cnt[2] = pair_count(xh, yh);
        cnt[3] = pair_count(xh >> 16, yh >> 16);
    }
}

template <int G, typename OutT>
__global__ __launch_bounds__(kBlock, 3)
void matrix_smh_narrow_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int r0, int r1, int n_y, int n_tiles, long long n_units, MatrixOut o) {
    constexpr int Q = kMatrixSmhNarrowQ;
    constexpr int LPR = kWave / G;                     // u64x2 (lanes) per sketch row: m = 2 LPR
    constexpr int AHEAD = kStreamAhead;
    constexpr int RING = AHEAD + 1;
    static_assert(kMatrixSpan % G == 0, "a span is whole wave loads");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int sub = lane & (LPR - 1), grp = lane / LPR;                       // this lane's place in its row, its row in the load
    const double m_f = (double)(2 * LPR);
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
        u64x2 q[Q];
        int acc[Q];
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            q[a] = X[(long long)min(i0 + a, r1 - 1) * LPR + sub];             // every lane group holds the whole row; rows past the slab: a valid row, never stored
            acc[a] = 0;
        }
        u64x2 ring[RING];
        // rows kk .. kk + G - 1, one per lane group: 1 KiB in a row of the array, except that a group past the span re-reads row ke - 1
        auto load_rows = [&](u64x2& dst, int kk) { dst = Y[(long long)min(kk + grp, ke - 1) * LPR + sub]; };
        auto compare_rows = [&](const u64x2& cand, int kk) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                int cnt[G];
                matrix_smh_narrow_counts<G>(q[a], cand, cnt);
#pragma unroll
                for (int g = 0; g < G; ++g) acc[a] = matrix_smh_writelane(cnt[g], kk - k0 + g, acc[a]);      // (lanes >= ke - k0 are never stored)
            }
        };
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) load_rows(ring[s], k0 + s * G);
        for (int k = k0; k < ke; k += RING * G) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                const int kk = k + s * G;
                if (kk >= ke) break;
                load_rows(ring[(s + AHEAD) % RING], kk + AHEAD * G);
                compare_rows(ring[s], kk);
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

// ---- wide rows: m = 1024 C, C = 2 .. 8 ------------------------------------------------------------------------------------------------
// the count of one chunk of 128 NCH buckets of a query row against the same chunk of a candidate row: 2 NCH v_cmp_eq_u64 and as many
// s_bcnt1_i32_b64 (the compare step of matrix_smh_kernel, as a function)
template <int NCH>
__device__ __forceinline__ int matrix_smh_chunk_count(const u64x2 (&q)[NCH], const u64x2 (&cand)[NCH]) {
    int cnt = 0;
#pragma unroll
    for (int c = 0; c < NCH; ++c) cnt += __popcll(__ballot(cand[c].x == q[c].x)) + __popcll(__ballot(cand[c].y == q[c].y));
    return cnt;
}

template <typename OutT>
__global__ __launch_bounds__(kBlock, 2)
void matrix_smh_wide_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_chunks, int r0, int r1, int n_y, int n_tiles, long long n_units, MatrixOut o) {
    constexpr int NCH = kMatrixSmhWideNch;
    constexpr int Q = matrix_smh_q(NCH);
    constexpr int CHV = NCH * kWave;                   // u64x2 per chunk of a row
    const long long pitch = (long long)n_chunks * CHV; // u64x2 per sketch row
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const double m_f = (double)(2 * CHV) * (double)n_chunks;
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
        auto load_queries = [&](int c) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const u64x2* row = X + (long long)min(i0 + a, r1 - 1) * pitch + (long long)c * CHV + lane;     // rows past the slab: a valid row, never stored
#pragma unroll
                for (int h = 0; h < NCH; ++h) q[a][h] = row[h * kWave];
            }
        };
        int acc[Q];                                                          // lane l: the running count of column k0 + l
#pragma unroll
        for (int a = 0; a < Q; ++a) acc[a] = 0;
        // ONE stream of (chunk, candidate row) steps, chunk-major, through a ring of two: the step behind the one compared is in flight,
        // also where that is the first row of the next chunk
        u64x2 ring[2][NCH];
        int pc = 0, pk = k0;                                                 // the step to fetch next (wave-uniform)
        auto prefetch = [&](u64x2 (&dst)[NCH]) {
            const u64x2* row = Y + (long long)pk * pitch + (long long)pc * CHV + lane;
#pragma unroll
            for (int h = 0; h < NCH; ++h) dst[h] = row[h * kWave];
            if (pk + 1 < ke) ++pk;
            else if (pc + 1 < n_chunks) { pk = k0; ++pc; }                   // (behind the last step: that step again)
        };
        int cc = 0, ck = k0;                                                 // the step to compare next
        auto compare_row = [&](const u64x2 (&cand)[NCH]) {
            const int col = ck - k0;
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const int cnt = matrix_smh_chunk_count<NCH>(q[a], cand) + __builtin_amdgcn_readlane(acc[a], col);
                acc[a] = matrix_smh_writelane(cnt, col, acc[a]);
            }
            if (++ck == ke) {
                ck = k0;
                if (++cc < n_chunks) load_queries(cc);
            }
        };
        const int steps = n_chunks * (ke - k0);
        prefetch(ring[0]);
        load_queries(0);
        for (int t = 0; t < steps; t += 2) {
            prefetch(ring[1]);
            compare_row(ring[0]);
            if (t + 1 >= steps) break;
            prefetch(ring[0]);
            compare_row(ring[1]);
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

}  // namespace

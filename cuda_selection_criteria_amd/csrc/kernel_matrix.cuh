// kernel_matrix.cuh -- matrix_kernel: the HLL-14 union size U or the Jaccard estimate J of EVERY pair as a dense array
// (selhip_ctx_matrix / selhip_ctx_query_matrix, abi_matrix.inc).
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace), behind kernel_dense.cuh and
// host_plan.hpp: the middle of a unit is dense_select_kernel's through the same device functions, the slab and mirror rules are host_plan's.
//   * unit = four neighbouring rows (one per wave) x a span of 64 consecutive columns, spans dealt to the XCDs round robin -- as in
//     dense_select_kernel, but over the whole rectangle: no triangle of ranges, no CB cut-off, no skip of empty sketches;
//   * per column: bs_load + bs_pair_hist into column (k - span start) of the wave's pitch-65 LDS tile, then lane = column: dense_estimate
//     on its own column gives U; J = (e_row + e_col - U) / U (selection.cpp:287) from the cardinalities truncated here (selhip::trunc_card);
//   * the tail is a typed store: out[pos_r * ld + pos_c], 64 consecutive columns of one row per wave -- no ballot, no counter, no atomic.
// A self matrix (X = Y) computes every pair once: row i of the slab [r0, r1) takes the columns [0, r0) u [i, n) (matrix_computes) and
// stores the cells i < k < r1 a second time at (k, i) (matrix_mirrors).  The cell is bit-symmetric -- e_a + e_b commutes, the
// histogram is that of a register-wise maximum, kp = max(gmax_a, gmax_b) + 1 -- so the mirror is a saving, not a definition.
// The diagonal is computed like any cell (U(i, i), I(i, i)); the Jaccard measure and the two containments store exactly 1.0 there.
// Measures: U itself, or selhip::pair_value (pair_value.hpp) of U and the two truncated cardinalities -- J, the intersection estimate I,
// the containment I / e_row (not symmetric: the mirrored store at (k, i) writes I / e_k from the same U) and the max containment
// I / min(e_row, e_col); a containment with an empty sketch in its denominator is NaN.
// Positions: row_pos (indexed by rank - r0) / col_pos (indexed by rank) are the HOST-VALIDATED copies of the caller's arrays, nullptr =
// the defaults rank - r0 / rank; every store address is 64-bit arithmetic on validated values.
#pragma once

namespace {

// one sketch set as the kernel reads it: bit planes, largest register value per genome, cardinalities as uploaded
struct MatrixSet {
    const uint32_t* bs;
    const uint8_t* gmax;
    const double* cards;
};

struct MatrixOut {
    void* out;                  // OutT [out_rows][ld]
    long long ld;               // elements
    const int* row_pos;         // [r1 - r0] or nullptr
    const int* col_pos;         // [n_y] or nullptr
    int measure;                // SELHIP_MEASURE_*
    int self;                   // X = Y: every pair once, mirrored stores (mirror = 0: the test switch "matrix_mirror", upper triangle only)
    int mirror;
};

template <int NB, bool FMA, typename OutT>
__global__ __launch_bounds__(kBlock, NB <= 5 ? 4 : 2)
void matrix_kernel(MatrixSet X, MatrixSet Y, int r0, int r1, int n_y, int n_tiles, long long n_units, double relerr_scaled, MatrixOut o) {
    __shared__ uint32_t tile_all[kWavesPerBlock][32 * kDensePitch];
    static_assert(kMatrixSpan == kDenseSpan, "a span is one column of the dense tile per lane");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    uint32_t* const tile = tile_all[wave];
    // every column starts as the histogram of an empty sketch, as in dense_select_kernel: the columns a row does not compute keep
    // whatever valid histogram they held last, so all 64 lanes always run the estimator on real counts (and store nothing)
#pragma unroll 8
    for (int w = 0; w < 32; ++w) tile[w * kDensePitch + lane] = w == 0 ? (1u << 14) : 0u;
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");                   // a tile is private to its wave
    uint32_t* const my_word = tile + (bs_pidx(lane) + ((lane & 2) ? 16 : 0)) * kDensePitch;
    OutT* const out = static_cast<OutT*>(o.out);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long k0 = (8 * (j / n_tiles) + (u & 7)) * kMatrixSpan;
        if (k0 >= n_y) continue;
        const long long row = (long long)r0 + (j % n_tiles) * kWavesPerBlock + wave;
        if (row >= r1) continue;                                             // wave-uniform; the kernel has no block barrier
        const int i = (int)row;
        if (o.self && matrix_skips_span(r0, i, k0)) continue;                // wave-uniform too
        const int ke = (int)min((long long)n_y, k0 + kMatrixSpan);
        {
            uint32_t xa[NB][8];
            bs_load<NB>(X.bs, i, lane, xa);
            const int gx = (int)X.gmax[i];
#pragma unroll 1
            for (int y = (int)k0; y < ke; ++y) {
                if (o.self && !matrix_computes(r0, i, y)) continue;
                uint32_t yb[NB][8];
                bs_load<NB>(Y.bs, y, lane, yb);
                const int kp = max(gx, (int)Y.gmax[y]) + 1;                  // values this pair can hold: [0, kp)
                const uint32_t tot = bs_pair_hist<NB>(xa, yb, kp, lane);
                my_word[y - (int)k0] = tot;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        const int ky = (int)k0 + lane;
        const bool live = ky < ke && (!o.self || matrix_computes(r0, i, ky));
        const double t = dense_estimate<FMA>(tile + lane, relerr_scaled);
        if (live) {
            double v = t, vm = t;                                            // the cell and its mirror image (k, i)
            if (o.measure != SELHIP_MEASURE_UNION) {
                const double e1 = (double)selhip::trunc_card(X.cards[i]), e2 = (double)selhip::trunc_card(Y.cards[ky]);
                v = vm = selhip::pair_value(o.measure, e1, e2, t);           // selection.cpp:287 (pair_value.hpp)
                // the one measure that is not symmetric: the mirrored cell is the share of genome k, from the same U
                if (o.measure == SELHIP_MEASURE_CONTAINMENT) vm = selhip::pair_value(SELHIP_MEASURE_CONTAINMENT, e2, e1, t);
                if (o.self && ky == i && o.measure != SELHIP_MEASURE_INTERSECTION) v = 1.0;
            }
            const size_t pos_r = (size_t)(o.row_pos ? o.row_pos[i - r0] : i - r0), pos_c = (size_t)(o.col_pos ? o.col_pos[ky] : ky);
            out[pos_r * (size_t)o.ld + pos_c] = (OutT)v;
            if (o.self && o.mirror && matrix_mirrors(i, ky, r1)) {
                const size_t m_r = (size_t)(o.row_pos ? o.row_pos[ky - r0] : ky - r0), m_c = (size_t)(o.col_pos ? o.col_pos[i] : i);
                out[m_r * (size_t)o.ld + m_c] = (OutT)vm;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");               // the next unit's stores come after these reads
    }
}

}  // namespace

// abi_matrix.inc -- the C ABI of the dense matrices (include/selection_hip.h section 2f): selhip_ctx_matrix / selhip_ctx_query_matrix.
// (selhip_ctx_linkage fills its scratch through matrix_call too, under its own timer and name: as_timer, as_what.)
// One launch of matrix_kernel (kernel_matrix.cuh; the HLL measures) or of a kernel of kernel_matrix_smh.cuh (the SuperMinHash measures)
// behind the host-side validation of every position; touches none of the passes' state (result list, counters, statistics, top-k,
// signature cache).
// Included by selection_kernels.hip.

namespace {

// the positions of ranks [b, e) -- the caller's (src, indexed by rank) or the defaults rank - b -- checked against [0, limit) into
// `checked` (indexed by rank - b); the first offending rank through *bad
bool matrix_positions(const int32_t* src, int64_t b, int64_t e, int64_t limit, std::vector<int>* checked, int64_t* bad) {
    if (src) checked->resize((size_t)(e - b));
    for (int64_t r = b; r < e; ++r) {
        const int64_t pos = src ? (int64_t)src[r] : r - b;
        if (pos < 0 || pos >= limit) { *bad = r; return false; }
        if (src) (*checked)[(size_t)(r - b)] = (int)pos;
    }
    return true;
}

hipError_t launch_matrix(bool fma, int dtype, hipStream_t st, int khi, const MatrixSet& X, const MatrixSet& Y, int r0, int r1, int n_y, const MatrixOut& o) {
    const MatrixUnits mu = matrix_units((long long)r1 - r0, n_y);
    if (mu.n_units <= 0) return hipSuccess;
    if (mu.n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<long long>(mu.n_units, 0x7FFFFFF8ll);          // (a multiple of 8; beyond it blocks take several units)
    const double rs = relerr_scaled_for(14);
    with_flag(fma, [&](auto F) { with_flag(dtype == SELHIP_F32, [&](auto F32) {
        using OutT = std::conditional_t<decltype(F32)::value, float, double>;
#define SELHIP_MATRIX_LAUNCH(NB) hipLaunchKernelGGL((matrix_kernel<NB, decltype(F)::value, OutT>), dim3(grid), dim3(kBlock), 0, st, X, Y, r0, r1, n_y, \
                                                    (int)mu.n_tiles, mu.n_units, rs, o)
        switch (bs_planes(khi)) {
            case 4:  SELHIP_MATRIX_LAUNCH(4); break;
            case 5:  SELHIP_MATRIX_LAUNCH(5); break;
            default: SELHIP_MATRIX_LAUNCH(6);
        }
#undef SELHIP_MATRIX_LAUNCH
    }); });
    return hipGetLastError();
}

// the SuperMinHash measures: the fast kernel where matrix_smh_fast(m), else the generic one; *fast_out = which.  (The fast kernel's
// 16-byte loads need 16-byte aligned rows: selhip_ctx_attach / _attach_queries refuse other pointers, uploads allocate their own.)  The grid is the unit count (one block per unit, capped as above).
hipError_t launch_matrix_smh(int dtype, hipStream_t st, const u64* X, const u64* Y, int m, int r0, int r1, int n_y, const MatrixOut& o, int* fast_out) {
    const bool fast = matrix_smh_fast(m);
    *fast_out = fast ? 1 : 0;
    const MatrixUnits mu = matrix_units((long long)r1 - r0, n_y, fast ? matrix_smh_tile_rows(m) : kWavesPerBlock);
    if (mu.n_units <= 0) return hipSuccess;
    if (mu.n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)std::min<long long>(mu.n_units, 0x7FFFFFF8ll);
    with_flag(dtype == SELHIP_F32, [&](auto F32) {
        using OutT = std::conditional_t<decltype(F32)::value, float, double>;
        if (!fast) {
            hipLaunchKernelGGL((matrix_smh_generic_kernel<OutT>), dim3(grid), dim3(kBlock), 0, st, X, Y, m, r0, r1, n_y, (int)mu.n_tiles, mu.n_units, o);
            return;
        }
#define SELHIP_MATRIX_SMH_LAUNCH(NCH) hipLaunchKernelGGL((matrix_smh_kernel<NCH, OutT>), dim3(grid), dim3(kBlock), 0, st, (const u64x2*)X, (const u64x2*)Y, \
                                                         r0, r1, n_y, (int)mu.n_tiles, mu.n_units, o)
        switch (m / 128) {
            case 1:  SELHIP_MATRIX_SMH_LAUNCH(1); break;
            case 2:  SELHIP_MATRIX_SMH_LAUNCH(2); break;
            case 4:  SELHIP_MATRIX_SMH_LAUNCH(4); break;
            default: SELHIP_MATRIX_SMH_LAUNCH(8);
        }
#undef SELHIP_MATRIX_SMH_LAUNCH
    });
    return hipGetLastError();
}

int matrix_call(selhip_ctx* c, bool query, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev,
                int64_t out_rows, int64_t out_cols, int64_t ld, const int32_t* row_pos, const int32_t* col_pos, int as_timer = -1, const char* as_what = nullptr) {
    if (!c) return SELHIP_E_BADARG;
    const char* const what = as_what ? as_what : query ? "selhip_ctx_query_matrix" : "selhip_ctx_matrix";
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", what); return SELHIP_E_STATE; }
    const bool smh = measure == SELHIP_MEASURE_SMH_MATCHES || measure == SELHIP_MEASURE_SMH_JACCARD;
    const bool share = measure == SELHIP_MEASURE_INTERSECTION || measure == SELHIP_MEASURE_CONTAINMENT || measure == SELHIP_MEASURE_MAX_CONTAINMENT;
    if (measure != SELHIP_MEASURE_JACCARD && measure != SELHIP_MEASURE_UNION && !share && !smh) { set_err(&c->err, "%s: bad measure %d", what, measure); return SELHIP_E_BADARG; }
    if (dtype != SELHIP_F64 && dtype != SELHIP_F32) { set_err(&c->err, "%s: bad dtype %d", what, dtype); return SELHIP_E_BADARG; }
    if (query && c->q.n < 0) { set_err(&c->err, "%s: no queries attached (selhip_ctx_upload_queries / _attach_queries)", what); return SELHIP_E_BADARG; }
    const int64_t n_x = query ? c->q.n : c->n, n_y = c->n;
    if (r0 > r1) { set_err(&c->err, "%s: r0 (%lld) > r1 (%lld)", what, (long long)r0, (long long)r1); return SELHIP_E_BADARG; }
    if (r0 < 0 || r1 > n_x) { set_err(&c->err, "%s: rows [%lld, %lld) outside [0, %lld)", what, (long long)r0, (long long)r1, (long long)n_x); return SELHIP_E_BADARG; }
    // the rule of accept_dense: p = 14 sketches with their bit planes resident (there is no byte-row form of the kernel)
    // (the SuperMinHash measures read the bucket rows alone: any p_hll, planes or none)
    if (!smh && (c->p != 14 || (n_y > 0 && !use_bitslices(c)) || (query && n_x > 0 && c->q.planes.khi <= 0))) {
        set_err(&c->err, "%s (dense matrix) needs p_hll = 14 sketches and their bit planes (p_hll = %d, hist_algo = %d)", what, c->p, c->hist_algo);
        return SELHIP_E_BADARG;
    }
    const size_t elem = dtype == SELHIP_F32 ? 4 : 8;
    if ((uintptr_t)out_dev & (elem - 1)) { set_err(&c->err, "%s: the output buffer must be aligned to its %zu-byte elements", what, elem); return SELHIP_E_BADARG; }
    if (out_rows < 0 || out_cols < 0 || ld < out_cols) {
        set_err(&c->err, "%s: ld (%lld) < out_cols (%lld), or a negative extent (out_rows %lld)", what, (long long)ld, (long long)out_cols, (long long)out_rows);
        return SELHIP_E_BADARG;
    }
    if (n_y == 0 || r0 == r1) return SELHIP_OK;                  // nothing to write: no buffer needed, no position read
    if (smh ? (!c->d_aux || c->m <= 0 || (query && !c->q.d_aux)) : (!c->d_cards || (query && !c->q.d_cards))) { set_err(&c->err, "%s before upload/attach", what); return SELHIP_E_STATE; }
    if (!out_dev) { set_err(&c->err, "%s: null output buffer", what); return SELHIP_E_BADARG; }
    // every position -- the defaults too -- is checked here, and only the checked copies go to the device
    std::vector<int> rows_ok, cols_ok;
    int64_t bad = 0;
    if (!matrix_positions(row_pos, r0, r1, out_rows, &rows_ok, &bad)) {
        set_err(&c->err, "%s: row_pos[%lld] = %lld outside [0, out_rows = %lld)", what, (long long)bad, (long long)(row_pos ? row_pos[bad] : bad - r0), (long long)out_rows);
        return SELHIP_E_BADARG;
    }
    if (!matrix_positions(col_pos, 0, n_y, out_cols, &cols_ok, &bad)) {
        set_err(&c->err, "%s: col_pos[%lld] = %lld outside [0, out_cols = %lld)", what, (long long)bad, (long long)(col_pos ? col_pos[bad] : bad), (long long)out_cols);
        return SELHIP_E_BADARG;
    }
    HIPCHK(&c->err, hipSetDevice(c->device));
    if (row_pos) {
        HIPCHK(&c->err, c->mat_row_pos.ensure(rows_ok.size()));
        HIPCHK(&c->err, hipMemcpyAsync(c->mat_row_pos.p, rows_ok.data(), rows_ok.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    if (col_pos) {
        HIPCHK(&c->err, c->mat_col_pos.ensure(cols_ok.size()));
        HIPCHK(&c->err, hipMemcpyAsync(c->mat_col_pos.p, cols_ok.data(), cols_ok.size() * sizeof(int), hipMemcpyHostToDevice, c->stream));
    }
    if (row_pos || col_pos) HIPCHK(&c->err, hipStreamSynchronize(c->stream));      // rows_ok / cols_ok are read until here
    if (smh) {
        // a self matrix: every pair once with mirrored stores ("matrix_smh_form" 1, the default; "matrix_mirror" 0 keeps the pairs and
        // drops the mirrors), or the whole square like a query matrix ("matrix_smh_form" 3)
        const int self = !query && (c->matrix_smh_form == 1 || !c->matrix_mirror) ? 1 : 0;
        const MatrixOut o{out_dev, (long long)ld, row_pos ? c->mat_row_pos.p : nullptr, col_pos ? c->mat_col_pos.p : nullptr, measure, self, c->matrix_mirror};
        // timed as "matrix_smh", per call of these measures: "matrix" stays the HLL kernel's
        hipError_t e;
        {
            const int tm = as_timer >= 0 ? as_timer : T_MATRIX_SMH;
            TimedCall call(c, tm);
            TimerScope t(c, tm);
            e = launch_matrix_smh(dtype, c->stream, query ? c->q.d_aux : c->d_aux, c->d_aux, c->m, (int)r0, (int)r1, (int)n_y, o, &c->matrix_smh_path_used);
        }
        HIPCHK(&c->err, e);
        HIPCHK(&c->err, hipStreamSynchronize(c->stream));
        return SELHIP_OK;
    }
    const MatrixSet D{c->planes.bs.p, c->planes.gmax.p, c->d_cards};
    const MatrixSet X = query ? MatrixSet{c->q.planes.bs.p, c->q.planes.gmax.p, c->q.d_cards} : D;
    const int khi = query ? std::max(c->q.planes.khi, c->planes.khi) : c->planes.khi;
    const MatrixOut o{out_dev, (long long)ld, row_pos ? c->mat_row_pos.p : nullptr, col_pos ? c->mat_col_pos.p : nullptr, measure, query ? 0 : 1, c->matrix_mirror};
    // timed as "matrix", per matrix call: a counter of its own, timed_passes is the passes' (level 2 keeps this kernel's events)
    hipError_t e;
    {
        const int tm = as_timer >= 0 ? as_timer : T_MATRIX;
        TimedCall call(c, tm);
        TimerScope t(c, tm);
        e = launch_matrix(c->fp_mode == SELHIP_FP_FMA, dtype, c->stream, khi, X, D, (int)r0, (int)r1, (int)n_y, o);
    }
    HIPCHK(&c->err, e);
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

}  // namespace

extern "C" {

int selhip_ctx_matrix(selhip_ctx* c, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev,
                      int64_t out_rows, int64_t out_cols, int64_t ld, const int32_t* row_pos, const int32_t* col_pos) {
    return matrix_call(c, false, measure, dtype, r0, r1, out_dev, out_rows, out_cols, ld, row_pos, col_pos);
}

int selhip_ctx_query_matrix(selhip_ctx* c, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev,
                            int64_t out_rows, int64_t out_cols, int64_t ld, const int32_t* row_pos, const int32_t* col_pos) {
    return matrix_call(c, true, measure, dtype, r0, r1, out_dev, out_rows, out_cols, ld, row_pos, col_pos);
}

}  // extern "C"

// abi_adjacency.inc -- the C ABI of the sparse adjacency (include/selection_hip.h sections 2n and 3): selhip_ctx_adjacency over the
// result list a context holds, selhip_adjacency over a caller's list of entries.  Kernels in kernel_adjacency.cuh, host side in
// host_adjacency.hpp; touches none of the passes' state (result list, counters, statistics, top-k, signature cache) and nothing the
// graph calls report.
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_adjacency(selhip_ctx* c, int form, double min_value, const selhip_csr_t* out, int64_t cap, int64_t* nnz_out) {
    return adjacency_call(c, form, min_value, out, cap, nnz_out);
}

int selhip_adjacency(const selhip_int2_t* d_pairs, const double* d_values, int64_t n_pairs, int64_t n_rows, int64_t n_cols, int form, double min_value,
                     const selhip_csr_t* out, int64_t cap, int64_t* nnz_out, int64_t* long_rows_out, void* hip_stream) {
    const char* const who = "selhip_adjacency";
    if (const int rc = adj_check_args(nullptr, who, form, min_value, out, cap)) return rc;
    if (n_rows < 0 || n_rows > 0x7FFFFFFFll || n_cols < 0 || n_cols > 0x7FFFFFFFll || n_pairs < 0 || n_pairs > 0x7FFFFFFFll || (n_pairs > 0 && !d_pairs) ||
        (form == SELHIP_ADJ_SYMMETRIC && n_rows != n_cols)) {
        set_err(nullptr, "%s: 0 <= n_rows, n_cols, n_pairs <= 2^31 - 1, a non-null list where there is something to read, n_rows == n_cols in the symmetric form", who);
        return SELHIP_E_BADARG;
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    AdjResult res;
    int rc = SELHIP_OK;
    if (n_rows == 0 && n_pairs > 0) {
        res.bad = ClusterBad{(u64)n_pairs, 0};              // (every entry is out of range)
    } else if (n_pairs == 0) {
        rc = adj_empty(nullptr, st, n_rows, *out);
    } else {
        AdjScratch scratch;
        rc = adj_run(nullptr, st, scratch, AdjPairList{d_pairs, d_values}, (u64)n_pairs, n_rows, n_cols, form, min_value, *out, cap, &res);
        scratch.release();                                  // (the stream is idle behind the chain, or the chain failed)
    }
    if (rc && rc != SELHIP_E_OVERFLOW) return rc;
    if (res.bad.count) {
        set_err(nullptr, "the pair list holds %llu invalid entries (a row outside [0, %lld) or a column outside [0, %lld)); entry %llu is one", res.bad.count,
                (long long)n_rows, (long long)n_cols, res.bad.index);
        return SELHIP_E_BADARG;
    }
    if (nnz_out) *nnz_out = res.nnz;
    if (long_rows_out) *long_rows_out = res.long_rows;
    return rc;
}

}  // extern "C"

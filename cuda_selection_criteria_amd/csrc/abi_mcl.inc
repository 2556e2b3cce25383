// abi_mcl.inc -- the C ABI of the Markov clustering (include/selection_hip.h sections 2o and 3): selhip_ctx_mcl over the result list a
// context holds, selhip_mcl over a caller's symmetric CSR matrix.  Kernels in kernel_mcl.cuh, host side in host_mcl.hpp; touches none of
// the passes' state (result list, counters, statistics, top-k, signature cache) and nothing the graph and adjacency calls report.
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_mcl(selhip_ctx* c, double min_value, const selhip_mcl_params_t* params, const selhip_mcl_t* out) {
    return mcl_call(c, min_value, params, out);
}

int selhip_mcl(const selhip_csr_t* adj, int64_t n, int64_t nnz, const selhip_mcl_params_t* params, const selhip_mcl_t* out, void* hip_stream) {
    const char* const who = "selhip_mcl";
    if (n < 0 || n > 0x7FFFFFFFll || nnz < 0 || !adj || (n > 0 && !adj->d_row_ptr) || (nnz > 0 && (!adj->d_col || !adj->d_val || n == 0))) {
        set_err(nullptr, "%s: 0 <= n <= 2^31 - 1, nnz >= 0 (0 where n is 0), a selhip_csr_t with d_row_ptr, and d_col and d_val where there are entries", who);
        return SELHIP_E_BADARG;
    }
    if ((reinterpret_cast<uintptr_t>(adj->d_row_ptr) & 7) || (reinterpret_cast<uintptr_t>(adj->d_col) & 3) || (reinterpret_cast<uintptr_t>(adj->d_val) & 7)) {
        set_err(nullptr, "%s: d_row_ptr and d_val 8-byte aligned, d_col 4-byte aligned", who);
        return SELHIP_E_BADARG;
    }
    if (const int rc = mcl_check_out(nullptr, who, out, n)) return rc;
    selhip_mcl_params_t p;
    if (const int rc = mcl_params(nullptr, who, params, &p)) return rc;
    MclResult res;
    if (n > 0) {
        MclScratch scratch;
        const int rc = mcl_run(nullptr, (hipStream_t)hip_stream, scratch, adj->d_row_ptr, adj->d_col, adj->d_val, n, nnz, p, *out, &res);
        scratch.release();                                  // (the stream is idle behind the run, or the run failed)
        if (rc) return rc;
        if (const int bad = mcl_report_bad(nullptr, who, res, n)) return bad;
    }
    mcl_deliver(*out, res);
    return SELHIP_OK;
}

}  // extern "C"

// abi_nj.inc -- the C ABI of the neighbour-joining tree (include/selection_hip.h sections 2l and 3): selhip_ctx_neighbor_joining over
// the similarity matrix of a context's set, selhip_neighbor_joining over a caller's distance matrix.  Kernels in kernel_nj.cuh, host
// side in host_nj.hpp; touches none of the passes' state and none of the "matrix" / "matrix_smh" / "linkage" timers.
// Included by selection_kernels.hip, behind abi_linkage.inc.

extern "C" {

int selhip_ctx_neighbor_joining(selhip_ctx* c, int measure, selhip_nj_join_t* d_joins, int64_t* n_joins_out) {
    return nj_ctx_call(c, measure, d_joins, n_joins_out);
}

int selhip_neighbor_joining(double* d_dist, int64_t n, int64_t ld, selhip_nj_join_t* d_joins, int64_t* n_joins_out, void* hip_stream) {
    const char* const what = "selhip_neighbor_joining";
    if (n < 0 || n > 0x7FFFFFFFll || ld < n || (n > 1 && !d_dist) || (reinterpret_cast<uintptr_t>(d_dist) & 7) || (reinterpret_cast<uintptr_t>(d_joins) & 7)) {
        set_err(nullptr, "%s: 0 <= n <= 2^31 - 1, ld >= n, a non-null 8-byte aligned matrix where there is something to read, 8-byte aligned records", what);
        return SELHIP_E_BADARG;
    }
    if (n > 1) {
        const hipStream_t st = (hipStream_t)hip_stream;
        NjScratch s;
        const hipError_t e = nj_scratch(&s, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err(nullptr, "%s: scratch for %lld slots: %s", what, (long long)n, hipGetErrorString(e));
            return SELHIP_E_NOMEM;
        }
        ClusterBad bad{0, ~0ull};
        if (const int rc = nj_joins(nullptr, st, d_dist, n, ld, s, &bad)) return rc;
        if (bad.count) return nj_bad_cells(nullptr, what, bad, n);
        HIPCHK(nullptr, nj_outputs(st, s, n - 1, d_joins));
    }
    if (n_joins_out) *n_joins_out = std::max<int64_t>(n - 1, 0);
    return SELHIP_OK;
}

}  // extern "C"

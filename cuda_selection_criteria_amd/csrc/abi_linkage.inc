// abi_linkage.inc -- the C ABI of the dense-matrix hierarchy (include/selection_hip.h sections 2k and 3): selhip_ctx_linkage over the
// similarity matrix of a context's set, selhip_linkage over a caller's distance matrix.  Kernels in kernel_linkage.cuh, host side in
// host_linkage.hpp; touches none of the passes' state (result list, counters, statistics, top-k, signature cache) and none of the
// "matrix" / "matrix_smh" timers.
// Included by selection_kernels.hip, behind abi_matrix.inc (matrix_call).

extern "C" {

int selhip_ctx_linkage(selhip_ctx* c, int measure, int method, double max_height, const selhip_linkage_t* out, int64_t* n_merges_out) {
    return linkage_ctx_call(c, measure, method, max_height, out, n_merges_out);
}

int selhip_linkage(double* d_dist, int64_t n, int64_t ld, int method, double max_height, selhip_pair_t* d_merges, int32_t* d_size,
                   int64_t* n_merges_out, int64_t* rounds_out, void* hip_stream) {
    const char* const what = "selhip_linkage";
    if (n < 0 || n > 0x7FFFFFFFll || ld < n || (n > 1 && !d_dist) || (reinterpret_cast<uintptr_t>(d_dist) & 7)) {
        set_err(nullptr, "%s: 0 <= n <= 2^31 - 1, ld >= n, a non-null 8-byte aligned matrix where there is something to read", what);
        return SELHIP_E_BADARG;
    }
    if (const int rc = linkage_args(nullptr, what, method, max_height, d_merges)) return rc;
    LinkageCounts cnt;
    if (n <= 1) {
        linkage_trivial(n, &cnt);
    } else {
        const hipStream_t st = (hipStream_t)hip_stream;
        LinkageScratch s;
        const hipError_t e = linkage_scratch(&s, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err(nullptr, "%s: scratch for %lld slots: %s", what, (long long)n, hipGetErrorString(e));
            return SELHIP_E_NOMEM;
        }
        ClusterBad bad{0, ~0ull};
        if (const int rc = linkage_rounds(nullptr, st, d_dist, n, ld, method, max_height, s, &cnt, &bad)) return rc;
        if (bad.count) return linkage_bad_cells(nullptr, what, bad, n);
        HIPCHK(nullptr, linkage_outputs(st, s, cnt.merges, d_merges, d_size));
    }
    if (n_merges_out) *n_merges_out = cnt.merges;
    if (rounds_out) *rounds_out = cnt.rounds;
    return SELHIP_OK;
}

}  // extern "C"

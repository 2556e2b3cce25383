// abi_cluster.inc -- the C ABI of the single-linkage clusters (include/selection_hip.h sections 2g and 3): selhip_ctx_cluster over the
// result list a context holds, selhip_components over a caller's list of edges.  Kernels in kernel_cluster.cuh, host side in
// host_cluster.hpp; touches none of the passes' state (result list, counters, statistics, top-k, signature cache).
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_cluster(selhip_ctx* c, double min_value, int rep_rule, const selhip_clusters_t* out, int64_t* n_clusters_out) {
    return cluster_call(c, min_value, rep_rule, out, n_clusters_out);
}

int selhip_components(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, int32_t* d_label, void* hip_stream) {
    if (n < 0 || n > 0x7FFFFFFFll || n_pairs < 0 || (n_pairs > 0 && !d_pairs) || (n > 0 && !d_label)) {
        set_err(nullptr, "selhip_components: 0 <= n <= 2^31 - 1, n_pairs >= 0, and non-null arrays where there is something to read or write");
        return SELHIP_E_BADARG;
    }
    if (n == 0) {
        if (n_pairs == 0) return SELHIP_OK;
        set_err(nullptr, "the pair list holds %lld invalid entries (a vertex outside [0, 0)); entry 0 is one", (long long)n_pairs);
        return SELHIP_E_BADARG;
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_pairs == 0) {
        hipLaunchKernelGGL(cluster_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, (long long)n, d_label, (int*)nullptr, (int*)nullptr,
                           (int*)nullptr, (int*)nullptr);
        HIPCHK(nullptr, hipGetLastError());
        HIPCHK(nullptr, hipStreamSynchronize(st));
        return SELHIP_OK;
    }
    int* d_parent = nullptr;
    ClusterBad* d_bad = nullptr;
    ClusterBad bad{0, ~0ull};
    hipError_t e = hipMalloc((void**)&d_parent, (size_t)n * sizeof(int));
    if (e == hipSuccess) e = hipMalloc((void**)&d_bad, sizeof(ClusterBad));
    if (e == hipSuccess) e = cluster_unite_list(st, ClusterPairList{d_pairs}, (u64)n_pairs, n, d_parent, nullptr, nullptr, nullptr, nullptr, d_bad);
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // an invalid entry: the labels are not written
    if (e == hipSuccess && !bad.count) {
        hipLaunchKernelGGL(cluster_flatten_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, d_parent, (long long)n, d_label, (int*)nullptr, (uint32_t*)nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    if (d_parent) (void)hipFree(d_parent);
    if (d_bad) (void)hipFree(d_bad);
    HIPCHK(nullptr, e);
    if (bad.count) {
        set_err(nullptr, "the pair list holds %llu invalid entries (a vertex outside [0, %lld)); entry %llu is one", bad.count, (long long)n, bad.index);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

}  // extern "C"

// abi_cluster.inc -- the C ABI of the single-linkage clusters (include/selection_hip.h sections 2g and 3): selhip_ctx_cluster over the
// result list a context holds, selhip_components over a caller's list of edges.  Kernels in kernel_cluster.cuh, host side in
// host_cluster.hpp and host_graph.hpp; touches none of the passes' state (result list, counters, statistics, top-k, signature cache).
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
    if (n == 0) return graph_no_vertices(n_pairs);
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_pairs == 0) {
        hipLaunchKernelGGL(cluster_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, (long long)n, d_label, (int*)nullptr, (int*)nullptr,
                           (int*)nullptr, (int*)nullptr);
        HIPCHK(nullptr, hipGetLastError());
        HIPCHK(nullptr, hipStreamSynchronize(st));
        return SELHIP_OK;
    }
    DevBlock<int, ClusterBad> scratch;                                         // parent[n], the tally of invalid entries
    ClusterBad bad{0, ~0ull};
    hipError_t e = scratch.alloc({(size_t)n, 1});
    if (e == hipSuccess) e = cluster_unite_list(st, GraphPairList{d_pairs}, (u64)n_pairs, n, scratch.part<0>(), nullptr, nullptr, nullptr, nullptr, scratch.part<1>());
    if (e == hipSuccess) e = hipMemcpyAsync(&bad, scratch.part<1>(), sizeof bad, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    // an invalid entry: the labels are not written
    if (e == hipSuccess && !bad.count) {
        hipLaunchKernelGGL(cluster_flatten_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, scratch.part<0>(), (long long)n, d_label, (int*)nullptr, (uint32_t*)nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(st);
    }
    HIPCHK(nullptr, e);
    return graph_bad_entries(bad, n);
}

}  // extern "C"

// abi_greedy.inc -- the C ABI of the greedy representative clusters (include/selection_hip.h sections 2h and 3):
// selhip_ctx_cluster_greedy over the result list a context holds, selhip_greedy_representatives over a caller's list of edges.  Kernels
// in kernel_greedy.cuh, host side in host_greedy.hpp and host_graph.hpp; touches none of the passes' state (result list, counters, statistics, top-k,
// signature cache) and nothing selhip_ctx_cluster reports.
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_cluster_greedy(selhip_ctx* c, double min_value, int order_rule, const uint32_t* d_priority, const selhip_greedy_t* out,
                              int64_t* n_clusters_out) {
    return greedy_call(c, min_value, order_rule, d_priority, out, n_clusters_out);
}

int selhip_greedy_representatives(const selhip_int2_t* d_pairs, int64_t n_pairs, int64_t n, const uint64_t* d_key, uint8_t* d_is_rep,
                                  int64_t* rounds_out, void* hip_stream) {
    if (n < 0 || n > 0x7FFFFFFFll || n_pairs < 0 || (n_pairs > 0 && !d_pairs) || (n > 0 && !d_is_rep)) {
        set_err(nullptr, "selhip_greedy_representatives: 0 <= n <= 2^31 - 1, n_pairs >= 0, and non-null arrays where there is something to read or write");
        return SELHIP_E_BADARG;
    }
    if (n == 0) {
        if (n_pairs == 0 && rounds_out) *rounds_out = 0;
        return graph_no_vertices(n_pairs);
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_pairs == 0) {
        hipLaunchKernelGGL(greedy_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, (long long)n, d_is_rep, (int*)nullptr, (double*)nullptr,
                           (int*)nullptr, (int*)nullptr, (int*)nullptr, (int*)nullptr);
        HIPCHK(nullptr, hipGetLastError());
        HIPCHK(nullptr, hipStreamSynchronize(st));
        if (rounds_out) *rounds_out = 1;
        return SELHIP_OK;
    }
    DevBlock<u64, int, int, uint32_t, ClusterBad> scratch;                     // key[n], state[n], blocked[n], the batch's counts, the tally of invalid entries
    ClusterBad bad{0, ~0ull};
    int64_t rounds = 0;
    int rc = SELHIP_OK;
    hipError_t e = scratch.alloc({(size_t)n, (size_t)n, (size_t)n, kGreedyBatch, 1});
    if (e == hipSuccess) {
        u64* const key = scratch.part<0>();
        int* const state = scratch.part<1>();
        int* const blocked = scratch.part<2>();
        ClusterBad* const d_bad = scratch.part<4>();
        const unsigned vgrid = cluster_vertex_grid(n);
        hipLaunchKernelGGL(greedy_clear_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, (int*)nullptr, d_bad);
        // NULL d_key: key = vertex, which is SELHIP_REP_MAX_RANK's
        hipLaunchKernelGGL(greedy_key_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, SELHIP_REP_MAX_RANK, (const int*)nullptr, (const uint32_t*)nullptr,
                           (const u64*)d_key, key, state, blocked, (u64*)nullptr, (int*)nullptr);
        e = hipGetLastError();
        if (e == hipSuccess) rc = greedy_rounds(nullptr, st, GraphPairList{d_pairs}, (u64)n_pairs, n, key, state, blocked, scratch.part<3>(), d_bad, &rounds);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(&bad, d_bad, sizeof bad, hipMemcpyDeviceToHost, st);
        if (e == hipSuccess && !rc) e = hipStreamSynchronize(st);
        // an invalid entry: the flags are not written
        if (e == hipSuccess && !rc && !bad.count) {
            hipLaunchKernelGGL(greedy_reps_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, (const int*)state, d_is_rep, (int*)nullptr, (uint32_t*)nullptr);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
    }
    if (rc) return rc;
    HIPCHK(nullptr, e);
    if (bad.count) return graph_bad_entries(bad, n);
    if (rounds_out) *rounds_out = rounds;
    return SELHIP_OK;
}

}  // extern "C"

// abi_forest.inc -- the C ABI of the maximum spanning forest (include/selection_hip.h sections 2j and 3): selhip_ctx_spanning_forest
// over the result list a context holds, selhip_spanning_forest over a caller's list of edges.  Kernels in kernel_forest.cuh, host side
// in host_forest.hpp and host_graph.hpp; touches none of the passes' state (result list, counters, statistics, top-k, signature cache) and nothing
// selhip_ctx_cluster or selhip_ctx_cluster_greedy report.
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_spanning_forest(selhip_ctx* c, double min_value, const selhip_forest_t* out, int64_t* n_edges_out) {
    return forest_call(c, min_value, out, n_edges_out);
}

int selhip_spanning_forest(const selhip_int2_t* d_pairs, const double* d_values, int64_t n_pairs, int64_t n, selhip_pair_t* d_edges, int32_t* d_label,
                           int64_t* n_edges_out, int64_t* rounds_out, void* hip_stream) {
    if (n < 0 || n > 0x7FFFFFFFll || n_pairs < 0 || (n_pairs > 0 && !d_pairs) || (d_edges && (reinterpret_cast<uintptr_t>(d_edges) & 15))) {
        set_err(nullptr, "selhip_spanning_forest: 0 <= n <= 2^31 - 1, n_pairs >= 0, a non-null list where there is something to read, d_edges 16-byte aligned");
        return SELHIP_E_BADARG;
    }
    if (n == 0) {
        if (n_pairs == 0 && n_edges_out) *n_edges_out = 0;
        if (n_pairs == 0 && rounds_out) *rounds_out = 0;
        return graph_no_vertices(n_pairs);
    }
    const hipStream_t st = (hipStream_t)hip_stream;
    if (n_pairs == 0) {
        hipLaunchKernelGGL(forest_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, (long long)n, d_label);
        HIPCHK(nullptr, hipGetLastError());
        HIPCHK(nullptr, hipStreamSynchronize(st));
        if (n_edges_out) *n_edges_out = 0;
        if (rounds_out) *rounds_out = 1;
        return SELHIP_OK;
    }
    // the emitted records, best_img[n], best_pair[n], the tally of invalid entries, parent[n], comp[n], the counters; rocPRIM's scratch
    // once the number of edges is known
    DevBlock<ForestEdge, u64, u64, ClusterBad, int, int, uint32_t> scratch;
    DevBlock<char> tmp;
    ClusterBad bad{0, ~0ull};
    int64_t rounds = 0, n_edges = 0;
    int rc = SELHIP_OK;
    hipError_t e = scratch.alloc({(size_t)std::max<int64_t>(n - 1, 1), (size_t)n, (size_t)n, 1, (size_t)n, (size_t)n, kForestWords});
    if (e == hipSuccess) {
        ForestEdge* const edges = scratch.part<0>();
        int* const comp = scratch.part<5>();
        rc = forest_rounds(nullptr, st, GraphValuedPairList{d_pairs, d_values}, (u64)n_pairs, n, scratch.part<4>(), comp, scratch.part<1>(), scratch.part<2>(), edges,
                           scratch.part<6>(), scratch.part<3>(), &rounds, &n_edges, &bad);
        // an invalid entry: nothing is written
        if (!rc && !bad.count) {
            size_t tmp_bytes = 0;
            if (d_edges && n_edges > 0) {
                e = forest_sort_bytes((size_t)n_edges, &tmp_bytes, st);
                if (e == hipSuccess) e = tmp.alloc({tmp_bytes + 256});
            }
            if (e == hipSuccess) e = forest_outputs(st, edges, n_edges, comp, n, tmp.base, tmp_bytes, d_edges, d_label);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
        }
    }
    if (rc) return rc;
    HIPCHK(nullptr, e);
    if (bad.count) return graph_bad_entries(bad, n);
    if (n_edges_out) *n_edges_out = n_edges;
    if (rounds_out) *rounds_out = rounds;
    return SELHIP_OK;
}

}  // extern "C"

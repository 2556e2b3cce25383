// host_cluster.hpp -- host side of the single-linkage clusters (kernel_cluster.cuh): the launches behind selhip_components and
// selhip_ctx_cluster, and the grids of the three graph calls with the grid hook of the test-suite.  Admission, the run of an admitted
// call and the scratch are host_graph.hpp's.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_graph.hpp); not a stand-alone header.
#pragma once

namespace {

// test hook ("cluster_blocks", process-wide: selhip_components has no context): > 0 fixes the grid of cluster_edges_kernel, so that a
// small list runs the grid-stride loop many times; 0 = sized from the list.  Atomic (relaxed: the value orders nothing, and the clusters
// are the same under every grid): one thread may set it through its context while other threads' graph calls read it
std::atomic<int> g_cluster_blocks{0};
// its sibling for the kernels that take a lane per vertex, row or slot ("vertex_blocks", process-wide and atomic for the same reasons):
// > 0 fixes the result of cluster_vertex_grid, so that a small n walks those kernels' grid-stride loops -- and the ballots, lane reads
// and per-cluster atomics at the end of each trip -- many times; 0 = sized from n.  It changes no answer: every such kernel strides by
// its own grid.  The row kernels of the merge by group (host_merge.hpp) take their grid here too
std::atomic<int> g_vertex_blocks{0};

unsigned cluster_edge_grid(u64 n_edges) {
    const int blocks = g_cluster_blocks.load(std::memory_order_relaxed);
    return blocks > 0 ? (unsigned)blocks : grid_for(n_edges, kBlock, kClusterMaxBlocks);
}
unsigned cluster_vertex_grid(int64_t n) {
    const int blocks = g_vertex_blocks.load(std::memory_order_relaxed);
    return blocks > 0 ? (unsigned)blocks : grid_for((u64)n, kBlock, 4096);
}

// parent[] initialised (with the tallies the caller wants cleared) and every edge of the list united, on st; nothing is waited for
template <class List>
hipError_t cluster_unite_list(hipStream_t st, const List& list, u64 n_edges, int64_t n, int* parent, int* degree, int* members,
                              uint32_t* flag, u64* key, ClusterBad* bad) {
    hipLaunchKernelGGL(cluster_init_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, st, parent, degree, members, flag, key, (long long)n, bad);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess || n_edges == 0) return e;
    hipLaunchKernelGGL((cluster_edges_kernel<List>), dim3(cluster_edge_grid(n_edges)), dim3(kBlock), 0, st, list, n_edges, (int)n, parent, degree, bad);
    return hipGetLastError();
}

// the launches of selhip_ctx_cluster behind its checks: n > 0 vertices, cnt > 0 records.  *bad_out = what the edge kernel refused
int cluster_launches(selhip_ctx* c, double min_value, int rule, const selhip_clusters_t& out, int64_t cnt, uint32_t* n_clusters, ClusterBad* bad_out) {
    const int64_t n = c->n;
    const size_t slots = (size_t)n + 1;                                        // one past the last vertex: the scan's total lands there
    const bool want_key = out.d_cluster_rep != nullptr;
    const bool want_degree = out.d_degree || (want_key && rule == SELHIP_REP_MAX_DEGREE);
    const bool want_members = out.d_cluster_size != nullptr;
    hipError_t e = c->gs.parent.ensure((size_t)n);
    if (e == hipSuccess && !out.d_label) e = c->gs.label.ensure((size_t)n);
    if (e == hipSuccess && want_degree && !out.d_degree) e = c->gs.degree.ensure((size_t)n);
    if (e == hipSuccess && want_members) e = c->gs.members.ensure((size_t)n);
    if (e == hipSuccess && want_key) e = c->gs.key.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.flag.ensure(slots);
    if (e == hipSuccess) e = c->gs.ids.ensure(slots);
    if (e == hipSuccess) e = c->gs.bad.ensure(1);
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, c->gs.flag.p, c->gs.ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream);
    if (e == hipSuccess) e = c->gs.tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "selhip_ctx_cluster: scratch for %lld genomes: %s", (long long)n, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    int* const label = out.d_label ? out.d_label : c->gs.label.p;
    int* const degree = !want_degree ? nullptr : out.d_degree ? out.d_degree : c->gs.degree.p;
    int* const members = want_members ? c->gs.members.p : nullptr;
    u64* const key = want_key ? c->gs.key.p : nullptr;
    const unsigned vgrid = cluster_vertex_grid(n);
    {
        TimerScope t(c, T_CLUSTER);
        HIPCHK(&c->err, cluster_unite_list(c->stream, GraphRecordList{c->results.p, min_value}, (u64)cnt, n, c->gs.parent.p, degree, members,
                                           c->gs.flag.p, key, c->gs.bad.p));
        hipLaunchKernelGGL(cluster_flatten_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, c->gs.parent.p, (long long)n, label, members, c->gs.flag.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->gs.tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->gs.tmp.p, tmp_bytes, c->gs.flag.p, c->gs.ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream));
        if (out.d_cluster || want_members || want_key) {
            hipLaunchKernelGGL(cluster_assign_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, label, members, degree, c->gs.ids.p, (long long)n, rule,
                               out.d_cluster, out.d_cluster_size, key);
            HIPCHK(&c->err, hipGetLastError());
        }
        if (want_key) {
            hipLaunchKernelGGL(cluster_rep_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, key, c->gs.ids.p, (long long)n, rule, out.d_cluster_rep);
            HIPCHK(&c->err, hipGetLastError());
        }
    }
    HIPCHK(&c->err, hipMemcpyAsync(n_clusters, c->gs.ids.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipMemcpyAsync(bad_out, c->gs.bad.p, sizeof(ClusterBad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int cluster_call(selhip_ctx* c, double min_value, int rule, const selhip_clusters_t* out, int64_t* n_clusters_out) {
    int rc = graph_admit(c, kClusterCall, out, min_value, [&] {
        if (rule == SELHIP_REP_MAX_DEGREE || rule == SELHIP_REP_MIN_RANK || rule == SELHIP_REP_MAX_RANK) return SELHIP_OK;
        set_err(&c->err, "selhip_ctx_cluster: bad rep_rule %d (SELHIP_REP_MAX_DEGREE, _MIN_RANK or _MAX_RANK)", rule);
        return SELHIP_E_BADARG;
    });
    if (rc) return rc;
    const int64_t n = c->n;
    uint32_t n_clusters = (uint32_t)n;
    rc = graph_run(c, kClusterCall,
                   [&] {   // n singletons
                       hipLaunchKernelGGL(cluster_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, c->stream, (long long)n, out->d_label,
                                          out->d_cluster, out->d_degree, out->d_cluster_size, out->d_cluster_rep);
                   },
                   [&](int64_t cnt, ClusterBad* bad) { return cluster_launches(c, min_value, rule, *out, cnt, &n_clusters, bad); });
    if (rc) return rc;
    c->clusters_last = (int)n_clusters;
    if (n_clusters_out) *n_clusters_out = (int64_t)n_clusters;
    return SELHIP_OK;
}

}  // namespace

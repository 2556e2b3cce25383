// host_cluster.hpp -- host side of the single-linkage clusters (kernel_cluster.cuh): the launches behind selhip_components and
// selhip_ctx_cluster, the context's scratch, and the grid hook of the test-suite.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_topk.hpp); not a stand-alone header.
#pragma once

namespace {

// test hook ("cluster_blocks", process-wide: selhip_components has no context): > 0 fixes the grid of cluster_edges_kernel, so that a
// small list runs the grid-stride loop many times; 0 = sized from the list
int g_cluster_blocks = 0;

unsigned cluster_edge_grid(u64 n_edges) { return g_cluster_blocks > 0 ? (unsigned)g_cluster_blocks : grid_for(n_edges, kBlock, kClusterMaxBlocks); }
unsigned cluster_vertex_grid(int64_t n) { return grid_for((u64)n, kBlock, 4096); }

void release_cluster(selhip_ctx* c) {
    c->cl_parent.release(); c->cl_label.release(); c->cl_degree.release(); c->cl_members.release(); c->cl_flag.release();
    c->cl_ids.release(); c->cl_key.release(); c->cl_bad.release(); c->cl_tmp.release();
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
    hipError_t e = c->cl_parent.ensure((size_t)n);
    if (e == hipSuccess && !out.d_label) e = c->cl_label.ensure((size_t)n);
    if (e == hipSuccess && want_degree && !out.d_degree) e = c->cl_degree.ensure((size_t)n);
    if (e == hipSuccess && want_members) e = c->cl_members.ensure((size_t)n);
    if (e == hipSuccess && want_key) e = c->cl_key.ensure((size_t)n);
    if (e == hipSuccess) e = c->cl_flag.ensure(slots);
    if (e == hipSuccess) e = c->cl_ids.ensure(slots);
    if (e == hipSuccess) e = c->cl_bad.ensure(1);
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, c->cl_flag.p, c->cl_ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream);
    if (e == hipSuccess) e = c->cl_tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "selhip_ctx_cluster: scratch for %lld genomes: %s", (long long)n, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    int* const label = out.d_label ? out.d_label : c->cl_label.p;
    int* const degree = !want_degree ? nullptr : out.d_degree ? out.d_degree : c->cl_degree.p;
    int* const members = want_members ? c->cl_members.p : nullptr;
    u64* const key = want_key ? c->cl_key.p : nullptr;
    const unsigned vgrid = cluster_vertex_grid(n);
    {
        TimerScope t(c, T_CLUSTER);
        HIPCHK(&c->err, cluster_unite_list(c->stream, ClusterRecordList{c->results.p, min_value}, (u64)cnt, n, c->cl_parent.p, degree, members,
                                           c->cl_flag.p, key, c->cl_bad.p));
        hipLaunchKernelGGL(cluster_flatten_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, c->cl_parent.p, (long long)n, label, members, c->cl_flag.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->cl_tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->cl_tmp.p, tmp_bytes, c->cl_flag.p, c->cl_ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream));
        if (out.d_cluster || want_members || want_key) {
            hipLaunchKernelGGL(cluster_assign_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, label, members, degree, c->cl_ids.p, (long long)n, rule,
                               out.d_cluster, out.d_cluster_size, key);
            HIPCHK(&c->err, hipGetLastError());
        }
        if (want_key) {
            hipLaunchKernelGGL(cluster_rep_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, key, c->cl_ids.p, (long long)n, rule, out.d_cluster_rep);
            HIPCHK(&c->err, hipGetLastError());
        }
    }
    HIPCHK(&c->err, hipMemcpyAsync(n_clusters, c->cl_ids.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipMemcpyAsync(bad_out, c->cl_bad.p, sizeof(ClusterBad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int cluster_call(selhip_ctx* c, double min_value, int rule, const selhip_clusters_t* out, int64_t* n_clusters_out) {
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "selhip_ctx_cluster: a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    if (!c->have_run) { set_err(&c->err, "selhip_ctx_cluster: the context holds no result list (run a pass first)"); return SELHIP_E_STATE; }
    if (c->last_was_query) {
        set_err(&c->err, "selhip_ctx_cluster: the result list is a query pass's, whose ranks live in two index spaces; cluster an all-pairs or pair-list pass");
        return SELHIP_E_STATE;
    }
    if (!out) { set_err(&c->err, "selhip_ctx_cluster: null selhip_clusters_t (its members may be null, the struct may not)"); return SELHIP_E_BADARG; }
    if (std::isnan(min_value)) { set_err(&c->err, "selhip_ctx_cluster: min_value is NaN (-INFINITY takes every record)"); return SELHIP_E_BADARG; }
    if (rule != SELHIP_REP_MAX_DEGREE && rule != SELHIP_REP_MIN_RANK && rule != SELHIP_REP_MAX_RANK) {
        set_err(&c->err, "selhip_ctx_cluster: bad rep_rule %d (SELHIP_REP_MAX_DEGREE, _MIN_RANK or _MAX_RANK)", rule);
        return SELHIP_E_BADARG;
    }
    const int64_t n = c->n, cnt = result_records(c);
    if (n > 0x7FFFFFFFll) { set_err(&c->err, "selhip_ctx_cluster takes up to 2^31 - 1 genomes"); return SELHIP_E_BADARG; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    // timed as "cluster", per cluster call: a counter of its own, like "matrix" (level 2 keeps these launches' events)
    const int dominant = c->dominant_timer;
    c->dominant_timer = T_CLUSTER;
    if (c->timing) c->timed_cluster_calls += 1;
    int rc = SELHIP_OK;
    uint32_t n_clusters = (uint32_t)n;
    ClusterBad bad{0, ~0ull};
    if (n == 0) {
        // nothing to write
    } else if (cnt == 0) {
        // no record, no edge: n singletons, written by the one launch
        {
            TimerScope t(c, T_CLUSTER);
            hipLaunchKernelGGL(cluster_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, c->stream, (long long)n, out->d_label, out->d_cluster,
                               out->d_degree, out->d_cluster_size, out->d_cluster_rep);
        }
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) { set_err(&c->err, "selhip_ctx_cluster: %s", hipGetErrorString(e)); rc = SELHIP_E_HIP; }
    } else {
        rc = cluster_launches(c, min_value, rule, *out, cnt, &n_clusters, &bad);
    }
    c->dominant_timer = dominant;
    if (rc) return rc;
    if (bad.count) {
        set_err(&c->err, "selhip_ctx_cluster: %llu records of the result list carry a rank outside [0, %lld); record %llu is one (internal error)",
                bad.count, (long long)n, bad.index);
        return SELHIP_E_HIP;
    }
    c->clusters_last = (int)n_clusters;
    if (n_clusters_out) *n_clusters_out = (int64_t)n_clusters;
    return SELHIP_OK;
}

}  // namespace

// host_greedy.hpp -- host side of the greedy representative clusters (kernel_greedy.cuh): the rounds and the launches behind
// selhip_greedy_representatives and selhip_ctx_cluster_greedy.  Admission, the run of an admitted call and the scratch are host_graph.hpp's.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_cluster.hpp, whose grids -- and so the
// "cluster_blocks" hook -- it uses); not a stand-alone header.
#pragma once

namespace {

// rounds enqueued between two looks at the UNDECIDED counts.  A round behind the one that decided the last vertex returns at its first
// instruction, so a batch's trailing rounds cost two empty launches each; a batch costs one 32-byte copy and one wait
constexpr int kGreedyBatch = 8;

// the rounds over a list whose key[], state[] (all UNDECIDED) and blocked[] (all 0) are ready on st, until no vertex is UNDECIDED.
// count: kGreedyBatch device words; bad: tallied by round 1.  *rounds_out = the first round after which no vertex was undecided.
// Waits for the stream after every batch
template <class List>
int greedy_rounds(std::string* err, hipStream_t st, const List& list, u64 n_edges, int64_t n, const u64* key, int* state, int* blocked,
                  uint32_t* count, ClusterBad* bad, int64_t* rounds_out) {
    const unsigned egrid = cluster_edge_grid(n_edges), vgrid = cluster_vertex_grid(n);
    uint32_t h_count[kGreedyBatch];
    for (int64_t done = 0; done < n; done += kGreedyBatch) {                      // at most n rounds decide n vertices
        HIPCHK(err, hipMemsetAsync(count, 0, sizeof h_count, st));
        for (int j = 0; j < kGreedyBatch; ++j) {
            const int round = (int)(done + j + 1);
            const uint32_t* prev = j ? count + j - 1 : nullptr;                   // (the batch before ended with vertices undecided)
            hipLaunchKernelGGL((greedy_edges_kernel<List>), dim3(egrid), dim3(kBlock), 0, st, list, n_edges, (int)n, key, state, blocked, round, prev,
                               round == 1 ? bad : (ClusterBad*)nullptr);
            hipLaunchKernelGGL(greedy_vertices_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, state, (const int*)blocked, round, prev, count + j);
        }
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipMemcpyAsync(h_count, count, sizeof h_count, hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        for (int j = 0; j < kGreedyBatch; ++j)
            if (h_count[j] == 0) { *rounds_out = done + j + 1; return SELHIP_OK; }
    }
    set_err(err, "greedy rounds: vertices undecided after %lld rounds (internal error)", (long long)n);
    return SELHIP_E_HIP;
}

// the launches of selhip_ctx_cluster_greedy behind its checks: n > 0 vertices, cnt > 0 records
int greedy_launches(selhip_ctx* c, double min_value, int rule, const uint32_t* d_priority, const selhip_greedy_t& out, int64_t cnt,
                    uint32_t* n_clusters, int64_t* rounds, ClusterBad* bad_out) {
    const int64_t n = c->n;
    const size_t slots = (size_t)n + 1;                                        // one past the last vertex: the scan's total lands there
    const bool want_degree = out.d_degree || rule == SELHIP_REP_MAX_DEGREE;
    const bool want_assign = out.d_rep_of || out.d_cluster || out.d_cluster_size;
    const bool want_best = want_assign || out.d_value;
    const bool want_members = out.d_cluster_size != nullptr;
    hipError_t e = c->gs.state.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.blocked.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.key.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.words.ensure(kGreedyBatch);
    if (e == hipSuccess && want_degree && !out.d_degree) e = c->gs.degree.ensure((size_t)n);
    if (e == hipSuccess && want_assign && !out.d_rep_of) e = c->gs.rep_of.ensure((size_t)n);
    if (e == hipSuccess && want_best) e = c->gs.best.ensure((size_t)n);
    if (e == hipSuccess && want_members) e = c->gs.members.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.flag.ensure(slots);
    if (e == hipSuccess) e = c->gs.ids.ensure(slots);
    if (e == hipSuccess) e = c->gs.bad.ensure(1);
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, c->gs.flag.p, c->gs.ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream);
    if (e == hipSuccess) e = c->gs.tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "selhip_ctx_cluster_greedy: scratch for %lld genomes: %s", (long long)n, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    int* const degree = !want_degree ? nullptr : out.d_degree ? out.d_degree : c->gs.degree.p;
    int* const rep_of = !want_assign ? nullptr : out.d_rep_of ? out.d_rep_of : c->gs.rep_of.p;
    u64* const best = want_best ? c->gs.best.p : nullptr;
    int* const members = want_members ? c->gs.members.p : nullptr;
    int* const state = c->gs.state.p;
    const GraphRecordList list{c->results.p, min_value};
    const unsigned vgrid = cluster_vertex_grid(n), egrid = cluster_edge_grid((u64)cnt);
    {
        TimerScope t(c, T_GREEDY);
        hipLaunchKernelGGL(greedy_clear_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, (long long)n, degree, c->gs.bad.p);
        if (want_degree)
            hipLaunchKernelGGL((greedy_degree_kernel<GraphRecordList>), dim3(egrid), dim3(kBlock), 0, c->stream, list, (u64)cnt, (int)n, degree);
        hipLaunchKernelGGL(greedy_key_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, (long long)n, rule, (const int*)degree, d_priority, (const u64*)nullptr,
                           c->gs.key.p, state, c->gs.blocked.p, best, members);
        HIPCHK(&c->err, hipGetLastError());
        const int rc = greedy_rounds(&c->err, c->stream, list, (u64)cnt, n, c->gs.key.p, state, c->gs.blocked.p, c->gs.words.p, c->gs.bad.p, rounds);
        if (rc) return rc;
        hipLaunchKernelGGL(greedy_reps_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, (long long)n, (const int*)state, (uint8_t*)nullptr, rep_of, c->gs.flag.p);
        if (want_best)
            hipLaunchKernelGGL((greedy_best_kernel<GraphRecordList>), dim3(egrid), dim3(kBlock), 0, c->stream, list, (u64)cnt, (int)n, (const int*)state, best);
        if (want_assign)
            hipLaunchKernelGGL((greedy_assign_kernel<GraphRecordList>), dim3(egrid), dim3(kBlock), 0, c->stream, list, (u64)cnt, (int)n, (const int*)state,
                               (const u64*)best, rep_of);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->gs.tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->gs.tmp.p, tmp_bytes, c->gs.flag.p, c->gs.ids.p, 0u, slots, rocprim::plus<uint32_t>(), c->stream));
        if (out.d_value || want_members)
            hipLaunchKernelGGL(greedy_members_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, (long long)n, (const int*)state, (const u64*)best, (const int*)rep_of,
                               out.d_value, members);
        if (out.d_cluster || out.d_cluster_size || out.d_cluster_rep)
            hipLaunchKernelGGL(greedy_write_kernel, dim3(vgrid), dim3(kBlock), 0, c->stream, (long long)n, (const int*)state, (const int*)rep_of,
                               (const uint32_t*)c->gs.ids.p, (const int*)members, out.d_cluster, out.d_cluster_size, out.d_cluster_rep);
        HIPCHK(&c->err, hipGetLastError());
    }
    HIPCHK(&c->err, hipMemcpyAsync(n_clusters, c->gs.ids.p + n, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipMemcpyAsync(bad_out, c->gs.bad.p, sizeof(ClusterBad), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int greedy_call(selhip_ctx* c, double min_value, int rule, const uint32_t* d_priority, const selhip_greedy_t* out, int64_t* n_clusters_out) {
    int rc = graph_admit(c, kGreedyCall, out, min_value, [&] {
        if (rule != SELHIP_REP_MAX_DEGREE && rule != SELHIP_REP_MIN_RANK && rule != SELHIP_REP_MAX_RANK && rule != SELHIP_REP_PRIORITY) {
            set_err(&c->err, "selhip_ctx_cluster_greedy: bad order_rule %d (SELHIP_REP_MAX_DEGREE, _MIN_RANK, _MAX_RANK or _PRIORITY)", rule);
            return SELHIP_E_BADARG;
        }
        if ((rule == SELHIP_REP_PRIORITY) != (d_priority != nullptr) && !(rule == SELHIP_REP_PRIORITY && c->n == 0)) {      // (no genome, no score to read)
            set_err(&c->err, "selhip_ctx_cluster_greedy: d_priority goes with SELHIP_REP_PRIORITY, and with no other order_rule (rule %d, d_priority %s)", rule,
                    d_priority ? "given" : "NULL");
            return SELHIP_E_BADARG;
        }
        return SELHIP_OK;
    });
    if (rc) return rc;
    const int64_t n = c->n;
    uint32_t n_clusters = (uint32_t)n;
    int64_t rounds = n ? 1 : 0;
    rc = graph_run(c, kGreedyCall,
                   [&] {   // n representatives
                       hipLaunchKernelGGL(greedy_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, c->stream, (long long)n, (uint8_t*)nullptr,
                                          out->d_rep_of, out->d_value, out->d_cluster, out->d_degree, out->d_cluster_size, out->d_cluster_rep);
                   },
                   [&](int64_t cnt, ClusterBad* bad) { return greedy_launches(c, min_value, rule, d_priority, *out, cnt, &n_clusters, &rounds, bad); });
    if (rc) return rc;
    c->greedy_clusters_last = (int)n_clusters;
    c->greedy_rounds_last = (int)rounds;
    if (n_clusters_out) *n_clusters_out = (int64_t)n_clusters;
    return SELHIP_OK;
}

}  // namespace

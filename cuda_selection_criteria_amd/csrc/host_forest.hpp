// host_forest.hpp -- host side of the maximum spanning forest (kernel_forest.cuh): the rounds, the sort and the launches behind
// selhip_spanning_forest and selhip_ctx_spanning_forest.  Admission, the run of an admitted call and the scratch are host_graph.hpp's.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_greedy.hpp; the grids -- and so the
// "cluster_blocks" hook -- are host_cluster.hpp's); not a stand-alone header.
#pragma once

namespace {

// rounds enqueued between two looks at the pick counts.  A round behind the one that picked nothing returns at its first instruction,
// so a batch's trailing rounds cost four empty launches each; a batch costs two small copies and one wait
constexpr int kForestBatch = 4;
constexpr int kForestWords = kForestBatch + 1;          // [0] the records emitted so far, [1 + j] the picks of the batch's round j

// the rounds over a list, on st, until one picks nothing: comp[] ends as the labels, edges[0 .. *edges_out) as the forest in the
// order the device emitted it.  words: kForestWords device words.  *rounds_out = the rounds, the empty one included; *bad_out = what
// round 1 refused.  Waits for the stream after every batch
template <class List>
int forest_rounds(std::string* err, hipStream_t st, const List& list, u64 n_edges, int64_t n, int* parent, int* comp, u64* best_img, u64* best_pair,
                  ForestEdge* edges, uint32_t* words, ClusterBad* bad, int64_t* rounds_out, int64_t* edges_out, ClusterBad* bad_out) {
    const unsigned egrid = cluster_edge_grid(n_edges), vgrid = cluster_vertex_grid(n);
    const uint32_t cap = (uint32_t)(n - 1);
    hipLaunchKernelGGL(forest_init_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, parent, comp, best_img, best_pair, words, bad);
    HIPCHK(err, hipGetLastError());
    int64_t most = 2;                                                              // ceil(log2 n) rounds that pick, the empty one, one to spare
    for (int64_t s = 1; s < n; s <<= 1) ++most;
    uint32_t h_words[kForestWords];
    for (int64_t done = 0; done < most; done += kForestBatch) {
        HIPCHK(err, hipMemsetAsync(words + 1, 0, kForestBatch * sizeof(uint32_t), st));
        for (int j = 0; j < kForestBatch; ++j) {
            const uint32_t* prev = j ? words + j : nullptr;                        // (the batch before ended with a round that picked)
            ClusterBad* const tally = done + j == 0 ? bad : (ClusterBad*)nullptr;
            hipLaunchKernelGGL((forest_best_kernel<List>), dim3(egrid), dim3(kBlock), 0, st, list, n_edges, (int)n, (const int*)comp, best_img, prev, tally);
            hipLaunchKernelGGL((forest_pick_kernel<List>), dim3(egrid), dim3(kBlock), 0, st, list, n_edges, (int)n, (const int*)comp, (const u64*)best_img,
                               best_pair, prev);
            hipLaunchKernelGGL(forest_hook_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, (const int*)comp, (const u64*)best_img,
                               (const u64*)best_pair, parent, edges, cap, words, prev);
            hipLaunchKernelGGL(forest_flatten_kernel, dim3(vgrid), dim3(kBlock), 0, st, (long long)n, (const int*)parent, comp, best_img, best_pair, prev,
                               words + 1 + j);
        }
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, st));
        if (done == 0) HIPCHK(err, hipMemcpyAsync(bad_out, bad, sizeof(ClusterBad), hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        for (int j = 0; j < kForestBatch; ++j)
            if (h_words[1 + j] == 0) {
                if (h_words[0] > cap) break;
                *rounds_out = done + j + 1;
                *edges_out = (int64_t)h_words[0];
                return SELHIP_OK;
            }
        if (h_words[0] > cap) break;
    }
    set_err(err, "spanning forest: no end after %lld rounds or more than n - 1 edges over %lld vertices (internal error)", (long long)most, (long long)n);
    return SELHIP_E_HIP;
}

// edges[0 .. f) in the device's order -> d_edges[0 .. f) in BEFORE order, and d_label = comp, on st; either output may be null.
// tmp / tmp_bytes: rocPRIM's scratch, as forest_sort_bytes sizes it for f records
hipError_t forest_sort_bytes(size_t f, size_t* bytes, hipStream_t st) {
    *bytes = 0;
    if (!f) return hipSuccess;
    return rocprim::merge_sort(nullptr, *bytes, (ForestEdge*)nullptr, (ForestEdge*)nullptr, f, ForestBefore(), st);
}
hipError_t forest_outputs(hipStream_t st, const ForestEdge* edges, int64_t f, const int* comp, int64_t n, void* tmp, size_t tmp_bytes,
                          selhip_pair_t* d_edges, int32_t* d_label) {
    hipError_t e = hipSuccess;
    if (d_edges && f > 0)
        e = rocprim::merge_sort(tmp, tmp_bytes, const_cast<ForestEdge*>(edges), reinterpret_cast<ForestEdge*>(d_edges), (size_t)f, ForestBefore(), st);
    if (e == hipSuccess && d_label) e = hipMemcpyAsync(d_label, comp, (size_t)n * sizeof(int), hipMemcpyDeviceToDevice, st);
    return e;
}

// the launches of selhip_ctx_spanning_forest behind its checks: n > 0 vertices, cnt > 0 records
int forest_launches(selhip_ctx* c, double min_value, const selhip_forest_t& out, int64_t cnt, int64_t* rounds, int64_t* n_edges, ClusterBad* bad_out) {
    const int64_t n = c->n;
    hipError_t e = c->gs.parent.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.label.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.key.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.best.ensure((size_t)n);
    if (e == hipSuccess) e = c->gs.words.ensure(kForestWords);
    if (e == hipSuccess) e = c->gs.bad.ensure(1);
    if (e == hipSuccess) e = c->gs.edges.ensure((size_t)std::max<int64_t>(n - 1, 1));
    if (e != hipSuccess) {
        set_err(&c->err, "selhip_ctx_spanning_forest: scratch for %lld genomes: %s", (long long)n, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    {
        TimerScope t(c, T_FOREST);
        const int rc = forest_rounds(&c->err, c->stream, GraphRecordList{c->results.p, min_value}, (u64)cnt, n, c->gs.parent.p, c->gs.label.p, c->gs.key.p,
                                     c->gs.best.p, c->gs.edges.p, c->gs.words.p, c->gs.bad.p, rounds, n_edges, bad_out);
        if (rc) return rc;
        if (bad_out->count) return SELHIP_OK;                                     // (the caller reports it; nothing is written)
        size_t tmp_bytes = 0;                                                     // (the stream is idle behind the rounds: the scratch may move)
        if (out.d_edges && *n_edges > 0) {
            HIPCHK(&c->err, forest_sort_bytes((size_t)*n_edges, &tmp_bytes, c->stream));
            HIPCHK(&c->err, c->gs.tmp.ensure(tmp_bytes + 256));
        }
        HIPCHK(&c->err, forest_outputs(c->stream, c->gs.edges.p, *n_edges, c->gs.label.p, n, c->gs.tmp.p, tmp_bytes, out.d_edges, out.d_label));
    }
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int forest_call(selhip_ctx* c, double min_value, const selhip_forest_t* out, int64_t* n_edges_out) {
    int rc = graph_admit(c, kForestCall, out, min_value, [] { return SELHIP_OK; });
    if (rc) return rc;
    if (out->d_edges && (reinterpret_cast<uintptr_t>(out->d_edges) & 15)) {
        set_err(&c->err, "selhip_ctx_spanning_forest: d_edges must be 16-byte aligned");
        return SELHIP_E_BADARG;
    }
    const int64_t n = c->n;
    int64_t rounds = n ? 1 : 0, n_edges = 0;
    rc = graph_run(c, kForestCall,
                   [&] {   // the identity labels
                       hipLaunchKernelGGL(forest_singletons_kernel, dim3(cluster_vertex_grid(n)), dim3(kBlock), 0, c->stream, (long long)n, out->d_label);
                   },
                   [&](int64_t cnt, ClusterBad* bad) { return forest_launches(c, min_value, *out, cnt, &rounds, &n_edges, bad); });
    if (rc) return rc;
    c->forest_rounds_last = (int)rounds;
    c->forest_edges_last = (int)n_edges;
    if (n_edges_out) *n_edges_out = n_edges;
    return SELHIP_OK;
}

}  // namespace

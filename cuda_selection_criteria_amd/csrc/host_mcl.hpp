// host_mcl.hpp -- host side of the Markov clustering (kernel_mcl.cuh; include/selection_hip.h section 2o): the parameters and their
// defaults, the scratch, the iteration loop behind selhip_ctx_mcl and selhip_mcl, the labels, and the context call's checks.  The loop
// waits for the stream once behind the input check, once per iteration -- the 8-byte chaos decides whether another is enqueued -- and
// once behind the labels.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_adjacency.hpp); not a stand-alone header.
#pragma once

namespace {

// what a run found: iterations, the last chaos, the clusters, the kernel class, what the input check refused (entries, rows)
struct MclResult { int64_t iters = 0, n_clusters = 0; double chaos = 0.0; int kclass = -1; ClusterBad bad[2] = {{0, ~0ull}, {0, ~0ull}}; };

// the caller's parameters with the defaults of section 2o filled in; SELHIP_E_BADARG outside their ranges
int mcl_params(std::string* err, const char* who, const selhip_mcl_params_t* in, selhip_mcl_params_t* p) {
    *p = in ? *in : selhip_mcl_params_t{};
    if (p->inflation == 0.0) p->inflation = 2.0;
    if (p->prune == 0.0) p->prune = 1e-4;
    if (p->chaos_tol == 0.0) p->chaos_tol = 1e-3;
    if (p->max_entries == 0) p->max_entries = 32;
    if (p->max_iters == 0) p->max_iters = 64;
    if (!(p->inflation > 1.0) || !std::isfinite(p->inflation) || !(p->prune > 0.0 && p->prune < 1.0) || !(p->chaos_tol > 0.0) || p->max_entries < 1 ||
        p->max_entries > SELHIP_MCL_MAX_ENTRIES || p->max_iters < 1) {
        set_err(err, "%s: inflation > 1 and finite, max_entries in 1 .. %d, prune in [0, 1), max_iters >= 1, chaos_tol > 0 (0 takes a field's default)", who,
                SELHIP_MCL_MAX_ENTRIES);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

int mcl_kclass(int K) { return K <= MclGeom<0>::kK ? 0 : K <= MclGeom<1>::kK ? 1 : 2; }

// the inverse of kernel_graph.cuh's graph_image, on the host
double mcl_chaos_value(u64 image) {
    const u64 b = (image >> 63) ? image & 0x7FFFFFFFFFFFFFFFull : ~image;
    double v;
    std::memcpy(&v, &b, sizeof v);
    return v;
}

template <int KCLASS>
void mcl_launch_step(hipStream_t st, const MclEll& in, const MclEll& out, int64_t n, int K, double r, double prune, u64* now, u64* next) {
    const unsigned grid = KCLASS == 0 ? grid_for((u64)n, kWavesPerBlock, 1u << 16) : grid_for((u64)n, 1, 1u << 16);
    const size_t lds = KCLASS == 0 ? 0 : mcl_lds_bytes(MclGeom<KCLASS>::kCap);
    hipLaunchKernelGGL(mcl_step_kernel<KCLASS>, dim3(grid), dim3(MclGeom<KCLASS>::kThreads), lds, st, in, out, (int)n, K, r, prune, now, next);
}

// The loop over an n x n matrix, n > 0, on st, and the labels.  SELHIP_OK with res->bad[.].count != 0: the input check refused the
// matrix, nothing was written and the caller reports it
int mcl_run(std::string* err, hipStream_t st, MclScratch& s, const int64_t* row_ptr, const int32_t* col, const double* val, int64_t n, int64_t nnz,
            const selhip_mcl_params_t& p, const selhip_mcl_t& out, MclResult* res) {
    const int K = p.max_entries;
    const size_t slots = (size_t)n + 1, cells = (size_t)n * (size_t)K;
    size_t tmp_bytes = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_bytes, (uint32_t*)nullptr, (uint32_t*)nullptr, 0u, slots, rocprim::plus<uint32_t>(), st);
    for (int b = 0; b < 2 && e == hipSuccess; ++b) {
        e = s.row[b].ensure(cells);
        if (e == hipSuccess) e = s.val[b].ensure(cells);
        if (e == hipSuccess) e = s.cnt[b].ensure((size_t)n);
    }
    if (e == hipSuccess) e = s.chaos.ensure(2);
    if (e == hipSuccess) e = s.bad.ensure(2);
    if (e == hipSuccess) e = s.parent.ensure((size_t)n);
    if (e == hipSuccess && !out.d_label) e = s.label.ensure((size_t)n);
    if (e == hipSuccess) e = s.flag.ensure(slots);
    if (e == hipSuccess) e = s.ids.ensure(slots);
    if (e == hipSuccess) e = s.tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(err, "mcl: scratch for %lld columns of %d entries: %s", (long long)n, K, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SELHIP_E_NOMEM : SELHIP_E_HIP;
    }
    // the two chaos slots (four words) and the two tallies cleared, the matrix checked
    hipLaunchKernelGGL(adj_init_kernel, dim3(1), dim3(kBlock), 0, st, reinterpret_cast<uint32_t*>(s.chaos.p), (u64)4, s.bad.p);
    hipLaunchKernelGGL(mcl_check_kernel, dim3(grid_for((u64)std::max(nnz, n), kBlock, 4096)), dim3(kBlock), 0, st, row_ptr, col, val, (long long)n, (long long)nnz, s.bad.p);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipMemcpyAsync(res->bad, s.bad.p, sizeof res->bad, hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    if (res->bad[0].count || res->bad[1].count) return SELHIP_OK;

    const MclEll ell[2] = {{s.row[0].p, s.val[0].p, s.cnt[0].p}, {s.row[1].p, s.val[1].p, s.cnt[1].p}};
    hipLaunchKernelGGL(mcl_start_kernel, dim3(grid_for((u64)n, 1, 1u << 16)), dim3(kMclStartBlock), mcl_lds_bytes(kMclStartCap), st, row_ptr, col, val, (int)n, K, ell[0]);
    HIPCHK(err, hipGetLastError());
    res->kclass = mcl_kclass(K);
    int cur = 0;
    for (int64_t it = 1; it <= (int64_t)p.max_iters; ++it) {
        u64* const now = s.chaos.p + (it & 1), * const next = s.chaos.p + ((it + 1) & 1);
        if (res->kclass == 0) mcl_launch_step<0>(st, ell[cur], ell[cur ^ 1], n, K, p.inflation, p.prune, now, next);
        else if (res->kclass == 1) mcl_launch_step<1>(st, ell[cur], ell[cur ^ 1], n, K, p.inflation, p.prune, now, next);
        else mcl_launch_step<2>(st, ell[cur], ell[cur ^ 1], n, K, p.inflation, p.prune, now, next);
        HIPCHK(err, hipGetLastError());
        u64 image = 0;
        HIPCHK(err, hipMemcpyAsync(&image, now, sizeof image, hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        cur ^= 1;
        res->iters = it; res->chaos = mcl_chaos_value(image);
        if (res->chaos <= p.chaos_tol) break;
    }
    // the stored entries of the final matrix as edges: the union-find, the labels and the dense ids of the single-linkage clusters
    int* const label = out.d_label ? out.d_label : s.label.p;
    const unsigned vgrid = cluster_vertex_grid(n);
    HIPCHK(err, cluster_unite_list(st, MclEdgeList{ell[cur].row, ell[cur].cnt, K}, (u64)cells, n, s.parent.p, nullptr, nullptr, s.flag.p, nullptr, s.bad.p));
    hipLaunchKernelGGL(cluster_flatten_kernel, dim3(vgrid), dim3(kBlock), 0, st, s.parent.p, (long long)n, label, (int*)nullptr, s.flag.p);
    HIPCHK(err, hipGetLastError());
    tmp_bytes = s.tmp.cap;
    HIPCHK(err, rocprim::exclusive_scan(s.tmp.p, tmp_bytes, s.flag.p, s.ids.p, 0u, slots, rocprim::plus<uint32_t>(), st));
    if (out.d_cluster) {
        hipLaunchKernelGGL(cluster_assign_kernel, dim3(vgrid), dim3(kBlock), 0, st, label, (const int*)nullptr, (const int*)nullptr, s.ids.p, (long long)n, 0,
                           out.d_cluster, (int*)nullptr, (u64*)nullptr);
        HIPCHK(err, hipGetLastError());
    }
    uint32_t n_clusters = 0;
    HIPCHK(err, hipMemcpyAsync(&n_clusters, s.ids.p + n, sizeof n_clusters, hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    res->n_clusters = (int64_t)n_clusters;
    return SELHIP_OK;
}

// what both entries ask of the result struct; who: the entry's name
int mcl_check_out(std::string* err, const char* who, const selhip_mcl_t* out, int64_t n) {
    if (!out || (n > 0 && !out->d_label)) { set_err(err, "%s: null selhip_mcl_t or d_label (d_cluster and the host pointers may be null)", who); return SELHIP_E_BADARG; }
    if ((reinterpret_cast<uintptr_t>(out->d_label) & 3) || (reinterpret_cast<uintptr_t>(out->d_cluster) & 3)) {
        set_err(err, "%s: d_label and d_cluster 4-byte aligned", who);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

int mcl_report_bad(std::string* err, const char* who, const MclResult& res, int64_t n) {
    if (res.bad[1].count) {
        set_err(err, "%s: %llu rows of d_row_ptr do not ascend from 0 to nnz; row %llu is one", who, res.bad[1].count, res.bad[1].index);
        return SELHIP_E_BADARG;
    }
    if (res.bad[0].count) {
        set_err(err, "%s: %llu entries carry a value that is not finite or is negative, a column outside [0, %lld) or a column that is not above its predecessor's "
                "in the row; entry %llu is one", who, res.bad[0].count, (long long)n, res.bad[0].index);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

void mcl_deliver(const selhip_mcl_t& out, const MclResult& res) {
    if (out.n_clusters) *out.n_clusters = res.n_clusters;
    if (out.iters) *out.iters = res.iters;
    if (out.chaos) *out.chaos = res.chaos;
}

int mcl_call(selhip_ctx* c, double min_value, const selhip_mcl_params_t* params, const selhip_mcl_t* out) {
    const char* const who = "selhip_ctx_mcl";
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", who); return SELHIP_E_STATE; }
    if (!c->have_run) { set_err(&c->err, "%s: the context holds no result list (run a pass first)", who); return SELHIP_E_STATE; }
    if (c->last_was_query) {
        set_err(&c->err, "%s: the result list is a query pass's, whose ranks live in two index spaces; cluster an all-pairs or pair-list pass", who);
        return SELHIP_E_STATE;
    }
    if (std::isnan(min_value)) { set_err(&c->err, "%s: min_value is NaN (-INFINITY takes every record)", who); return SELHIP_E_BADARG; }
    const int64_t n = c->n, cnt = result_records(c);
    if (const int rc = mcl_check_out(&c->err, who, out, n)) return rc;
    selhip_mcl_params_t p;
    if (const int rc = mcl_params(&c->err, who, params, &p)) return rc;
    if (n > 0x7FFFFFFFll || cnt > 0x7FFFFFFFll) { set_err(&c->err, "%s takes up to 2^31 - 1 genomes and records", who); return SELHIP_E_BADARG; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    MclResult res;
    if (n > 0) {
        const int64_t cap = 2 * cnt;
        hipError_t e = c->mcl.csr_row.ensure((size_t)n + 1);
        if (e == hipSuccess) e = c->mcl.csr_col.ensure((size_t)std::max<int64_t>(cap, 1));
        if (e == hipSuccess) e = c->mcl.csr_val.ensure((size_t)std::max<int64_t>(cap, 1));
        if (e != hipSuccess) {
            set_err(&c->err, "%s: the adjacency of %lld records: %s", who, (long long)cnt, hipGetErrorString(e));
            return e == hipErrorOutOfMemory ? SELHIP_E_NOMEM : SELHIP_E_HIP;
        }
        const selhip_csr_t csr{c->mcl.csr_row.p, c->mcl.csr_col.p, c->mcl.csr_val.p};
        AdjResult adj;
        TimedCall call(c, T_MCL);
        TimerScope t(c, T_MCL);
        int rc = cnt == 0 ? adj_empty(&c->err, c->stream, n, csr)
                          : adj_run(&c->err, c->stream, c->adj, AdjRecordList{c->results.p}, (u64)cnt, n, n, SELHIP_ADJ_SYMMETRIC, min_value, csr, cap, &adj);
        if (rc) return rc;
        if (adj.bad.count) {
            set_err(&c->err, "%s: %llu records of the result list carry a rank outside [0, %lld); record %llu is one (internal error)", who, adj.bad.count,
                    (long long)n, adj.bad.index);
            return SELHIP_E_HIP;
        }
        rc = mcl_run(&c->err, c->stream, c->mcl, csr.d_row_ptr, csr.d_col, csr.d_val, n, adj.nnz, p, *out, &res);
        if (rc) return rc;
        if (const int bad = mcl_report_bad(&c->err, who, res, n)) return bad;
    }
    c->mcl_iters_last = (int)std::min<int64_t>(res.iters, 0x7FFFFFFF);
    c->mcl_clusters_last = (int)res.n_clusters;
    c->mcl_kclass_last = res.kclass;                        // (-1 where no step kernel ran: a context without genomes)
    mcl_deliver(*out, res);
    return SELHIP_OK;
}

}  // namespace

// host_nj.hpp -- host side of the neighbour-joining tree (kernel_nj.cuh): the checks, the scratch and the joins behind
// selhip_neighbor_joining and selhip_ctx_neighbor_joining.
// Part of the kernel translation unit selection_kernels.hip (included there, behind host_linkage.hpp, whose declaration of matrix_call
// the context entry uses); not a stand-alone header.
#pragma once

namespace {

// the per-slot state, the two lists, the rows' bests, the records and what the pick publishes: one allocation
using NjScratch = DevBlock<uint8_t, double, int, int, double, int, selhip_nj_join_t, NjPick, ClusterBad>;

hipError_t nj_scratch(NjScratch* s, int64_t n) {
    const size_t m = (size_t)n;
    return s->alloc({m + 16, m + 2, m, m, m, m, (size_t)std::max<int64_t>(n - 1, 1), 1, 1});
}

// the n - 1 joins over D[n][ld], n >= 2, on st: mirror and validate (one wait: a refusal costs no join), the initial row sums, then
// scan / pick / update per join with nothing read back, and one wait at the end.  *bad_out: the cells refused (then nothing else has
// run).  Leaves the stream idle; the records lie in the scratch (part 6) for nj_outputs
int nj_joins(std::string* err, hipStream_t st, double* D, int64_t n, int64_t ld, const NjScratch& s, ClusterBad* bad_out) {
    uint8_t* const active = s.part<0>();
    double* const R = s.part<1>();
    int* const list[2] = {s.part<2>(), s.part<3>()};
    double* const best_q = s.part<4>();
    int* const best_b = s.part<5>();
    selhip_nj_join_t* const joins = s.part<6>();
    NjPick* const pick = s.part<7>();
    ClusterBad* const bad = s.part<8>();
    const unsigned vgrid = cluster_vertex_grid(n), tiles = (unsigned)((n + kLkTile - 1) / kLkTile);
    const bool wide = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(D) & 15) == 0;

    hipLaunchKernelGGL(nj_init_kernel, dim3(vgrid), dim3(kBlock), 0, st, (int)n, active, list[0], bad);
    hipLaunchKernelGGL(nj_mirror_kernel, dim3(tiles, tiles), dim3(kBlock), 0, st, D, (long long)ld, (int)n, bad);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipMemcpyAsync(bad_out, bad, sizeof(ClusterBad), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    if (bad_out->count) return SELHIP_OK;

    hipLaunchKernelGGL(nj_rowsum_kernel, dim3((unsigned)n), dim3(kNjSum), 0, st, (const double*)D, (long long)ld, (int)n, R);
    for (int64_t j = 0; j + 1 < n; ++j) {
        const int r = (int)(n - j);
        const double rm2 = (double)(r - 2);
        const int* const cur = list[j & 1];
        with_flag(wide, [&](auto W) {
            hipLaunchKernelGGL((nj_scan_kernel<decltype(W)::value>), dim3((unsigned)((r + kNjRows - 1) / kNjRows)), dim3(kBlock), 0, st, (const double*)D,
                               (long long)ld, (int)n, r, rm2, (const uint8_t*)active, (const double*)R, cur, best_q, best_b);
        });
        hipLaunchKernelGGL(nj_pick_kernel, dim3(1), dim3(kNjSum), 0, st, (const double*)D, (long long)ld, (int)n, r, rm2, (int)j, (const uint8_t*)active, R, cur,
                           (const double*)best_q, (const int*)best_b, joins, pick);
        if (r > 2)
            hipLaunchKernelGGL(nj_update_kernel, dim3(vgrid), dim3(kBlock), 0, st, D, (long long)ld, (int)n, r, (const NjPick*)pick, active, R, cur, list[(j + 1) & 1]);
    }
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipStreamSynchronize(st));
    return SELHIP_OK;
}

// the n - 1 records to the caller's array (may be null), on st; waits
hipError_t nj_outputs(hipStream_t st, const NjScratch& s, int64_t f, selhip_nj_join_t* d_joins) {
    hipError_t e = hipSuccess;
    if (d_joins && f > 0) e = hipMemcpyAsync(d_joins, s.part<6>(), (size_t)f * sizeof(selhip_nj_join_t), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

int nj_bad_cells(std::string* err, const char* entry, const ClusterBad& bad, int64_t n) {
    set_err(err, "%s: %llu cells of the upper triangle are NaN, +inf or -inf (a neighbour-joining tree takes finite distances); cell (%llu, %llu) is one",
            entry, bad.count, bad.index / (u64)n, bad.index % (u64)n);
    return SELHIP_E_BADARG;
}

int nj_ctx_call(selhip_ctx* c, int measure, selhip_nj_join_t* d_joins, int64_t* n_joins_out) {
    if (!c) return SELHIP_E_BADARG;
    const char* const what = "selhip_ctx_neighbor_joining";
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", what); return SELHIP_E_STATE; }
    if (measure != SELHIP_MEASURE_JACCARD && measure != SELHIP_MEASURE_MAX_CONTAINMENT && measure != SELHIP_MEASURE_SMH_JACCARD) {
        set_err(&c->err, "%s: measure %d is no symmetric similarity (SELHIP_MEASURE_JACCARD, _MAX_CONTAINMENT, _SMH_JACCARD)", what, measure);
        return SELHIP_E_BADARG;
    }
    if (reinterpret_cast<uintptr_t>(d_joins) & 7) { set_err(&c->err, "%s: d_joins must be 8-byte aligned", what); return SELHIP_E_BADARG; }
    const int64_t n = c->n;
    if (n > 0x7FFFFFFFll) { set_err(&c->err, "%s takes up to 2^31 - 1 genomes", what); return SELHIP_E_BADARG; }
    if (n == 1) {
        // (the refusals of a matrix call still hold for one genome; none has anything to refuse with no genome)
        if (const int rc = matrix_call(c, false, measure, SELHIP_F64, 0, 0, nullptr, 0, 0, 0, nullptr, nullptr, T_NJ, what)) return rc;
        // (an empty matrix call times nothing; "nj" is per call, so the call is counted here, with an empty scope on the stream)
        HIPCHK(&c->err, hipSetDevice(c->device));
        TimedCall call(c, T_NJ);
        TimerScope t(c, T_NJ);
    } else if (n > 1) {
        HIPCHK(&c->err, hipSetDevice(c->device));
        DevBlock<double> dist;
        NjScratch s;
        hipError_t e = dist.alloc({(size_t)n * (size_t)n});
        if (e == hipSuccess) e = nj_scratch(&s, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err(&c->err, "%s: %lld x %lld f64 cells of scratch: %s", what, (long long)n, (long long)n, hipGetErrorString(e));
            return SELHIP_E_NOMEM;
        }
        double* const D = dist.part<0>();
        if (const int rc = matrix_call(c, false, measure, SELHIP_F64, 0, n, D, n, n, n, nullptr, nullptr, T_NJ, what)) return rc;
        ClusterBad bad{0, ~0ull};
        int rc;
        {
            TimedCall call(c, T_NJ, false);                                       // (counted by the matrix call above)
            TimerScope t(c, T_NJ);
            hipLaunchKernelGGL(lk_distance_kernel, dim3(grid_for((u64)n * (u64)n, kBlock, 8192)), dim3(kBlock), 0, c->stream, D, (long long)n * n);
            rc = nj_joins(&c->err, c->stream, D, n, n, s, &bad);
        }
        if (rc) return rc;
        if (bad.count) return nj_bad_cells(&c->err, what, bad, n);                // (a similarity of -inf: no measure gives one)
        HIPCHK(&c->err, nj_outputs(c->stream, s, n - 1, d_joins));
    }
    if (n_joins_out) *n_joins_out = std::max<int64_t>(n - 1, 0);
    return SELHIP_OK;
}

}  // namespace

// host_linkage.hpp -- host side of the dense-matrix hierarchy (kernel_linkage.cuh): the checks, the scratch and the rounds behind
// selhip_linkage and selhip_ctx_linkage.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_forest.hpp and ahead of abi_matrix.inc, whose
// matrix_call the context entry fills its scratch with); not a stand-alone header.
#pragma once

namespace {

int matrix_call(selhip_ctx* c, bool query, int measure, int dtype, int64_t r0, int64_t r1, void* out_dev, int64_t out_rows, int64_t out_cols, int64_t ld,
                const int32_t* row_pos, const int32_t* col_pos, int as_timer, const char* as_what);

struct LinkageCounts { int64_t merges = 0, rounds = 0, rescans = 0, rowscans = 0; };

// the per-slot state, the round's pairs and the emitted records of one call: one allocation
using LinkageScratch = DevBlock<uint8_t, uint8_t, int, int, double, int, selhip_int2_t, ForestEdge, int, uint32_t, ClusterBad>;

hipError_t linkage_scratch(LinkageScratch* s, int64_t n) {
    const size_t m = (size_t)n;
    return s->alloc({m + 16, m, m, m, m, m, m / 2 + 1, (size_t)std::max<int64_t>(n - 1, 1), (size_t)std::max<int64_t>(n - 1, 1), kLkWords, 1});
}

bool linkage_method_ok(int method) { return method >= SELHIP_LINKAGE_SINGLE && method <= SELHIP_LINKAGE_WEIGHTED; }

// the rounds over D[n][ld], n >= 2, on st: mirror and validate, then scan / pair / update / book until a round that scanned every
// active row finds no pair.  *bad_out: the cells refused (then nothing else has run).  Leaves the stream idle; the records lie in the
// scratch (parts 7 and 8) for linkage_outputs
int linkage_rounds(std::string* err, hipStream_t st, double* D, int64_t n, int64_t ld, int method, double max_height, const LinkageScratch& s,
                   LinkageCounts* cnt, ClusterBad* bad_out) {
    uint8_t* const active = s.part<0>();
    uint8_t* const paired = s.part<1>();
    int* const size = s.part<2>();
    int* const nn = s.part<3>();
    double* const nd = s.part<4>();
    int* const list = s.part<5>();
    selhip_int2_t* const pairs = s.part<6>();
    ForestEdge* const merges = s.part<7>();
    int* const msize = s.part<8>();
    uint32_t* const words = s.part<9>();
    ClusterBad* const bad = s.part<10>();
    const unsigned vgrid = cluster_vertex_grid(n), tiles = (unsigned)((n + kLkTile - 1) / kLkTile), cols = (unsigned)((n + kBlock - 1) / kBlock);
    const bool wide = (ld & 1) == 0 && (reinterpret_cast<uintptr_t>(D) & 15) == 0;
    const uint32_t cap = (uint32_t)(n - 1);

    hipLaunchKernelGGL(lk_init_kernel, dim3(vgrid), dim3(kBlock), 0, st, (int)n, active, size, nn, nd, words, bad);
    hipLaunchKernelGGL(lk_mirror_kernel, dim3(tiles, tiles), dim3(kBlock), 0, st, D, (long long)ld, (int)n, bad);
    hipLaunchKernelGGL(lk_all_kernel, dim3(vgrid), dim3(kBlock), 0, st, (int)n, (const uint8_t*)active, list, words);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipMemcpyAsync(bad_out, bad, sizeof(ClusterBad), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    if (bad_out->count) return SELHIP_OK;

    int64_t n_active = n, n_dirty = n;
    uint32_t h_words[kLkWords];
    const int64_t most = 2 * (n - 1) + 1;
    while (cnt->rounds < most) {
        cnt->rounds += 1;
        cnt->rowscans += n_dirty;
        const bool full = n_dirty == n_active;
        with_flag(wide, [&](auto W) {
            hipLaunchKernelGGL((lk_scan_kernel<decltype(W)::value>), dim3((unsigned)n_dirty), dim3(kBlock), 0, st, (const double*)D, (long long)ld, (int)n,
                               (const uint8_t*)active, (const int*)list, nn, nd);
        });
        hipLaunchKernelGGL(lk_pair_kernel, dim3(1), dim3(kLkPairBlock), 0, st, (int)n, (const uint8_t*)active, (const int*)nn, (const double*)nd, (const int*)size,
                           max_height, paired, pairs, merges, msize, cap, words);
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipMemcpyAsync(h_words, words, sizeof h_words, hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        const int64_t n_pairs = h_words[1];
        if (n_pairs > n_active / 2 || h_words[2] > cap) break;
        if (n_pairs == 0) {
            if (full) { cnt->merges = h_words[2]; return SELHIP_OK; }
            cnt->rescans += 1;                                                    // stale caches (ties, an ulp of rounding): every row again
            hipLaunchKernelGGL(lk_all_kernel, dim3(vgrid), dim3(kBlock), 0, st, (int)n, (const uint8_t*)active, list, words);
            n_dirty = n_active;
            continue;
        }
        hipLaunchKernelGGL(lk_update_kernel, dim3(cols, (unsigned)std::min<int64_t>(n_pairs, 4096)), dim3(kBlock), 0, st, D, (long long)ld, (int)n, method,
                           (const uint8_t*)active, (const uint8_t*)paired, (const int*)nn, (const int*)size, (const selhip_int2_t*)pairs, (uint32_t)n_pairs);
        hipLaunchKernelGGL(lk_book_kernel, dim3(vgrid), dim3(kBlock), 0, st, (int)n, active, (const uint8_t*)paired, (const int*)nn, size, list, words);
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipMemcpyAsync(h_words, words, sizeof(uint32_t), hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        n_active -= n_pairs;
        n_dirty = h_words[0];
        if (n_dirty < n_pairs || n_dirty > n_active) break;
    }
    set_err(err, "linkage: no end after %lld rounds over %lld slots, or an impossible count (internal error)", (long long)cnt->rounds, (long long)n);
    return SELHIP_E_HIP;
}

// the first f records and sizes to the caller's arrays (either may be null), on st; waits
hipError_t linkage_outputs(hipStream_t st, const LinkageScratch& s, int64_t f, selhip_pair_t* d_merges, int32_t* d_size) {
    hipError_t e = hipSuccess;
    if (d_merges && f > 0) e = hipMemcpyAsync(d_merges, s.part<7>(), (size_t)f * sizeof(ForestEdge), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess && d_size && f > 0) e = hipMemcpyAsync(d_size, s.part<8>(), (size_t)f * sizeof(int), hipMemcpyDeviceToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e;
}

int linkage_bad_cells(std::string* err, const char* entry, const ClusterBad& bad, int64_t n) {
    set_err(err, "%s: %llu cells of the upper triangle are NaN or -inf; cell (%llu, %llu) is one", entry, bad.count, bad.index / (u64)n, bad.index % (u64)n);
    return SELHIP_E_BADARG;
}

// the checks both entries share; what = the entry's name
int linkage_args(std::string* err, const char* what, int method, double max_height, const void* d_merges) {
    if (!linkage_method_ok(method)) { set_err(err, "%s: bad method %d (SELHIP_LINKAGE_SINGLE, _COMPLETE, _AVERAGE, _WEIGHTED)", what, method); return SELHIP_E_BADARG; }
    if (std::isnan(max_height)) { set_err(err, "%s: max_height is NaN (INFINITY builds the whole hierarchy)", what); return SELHIP_E_BADARG; }
    if (d_merges && (reinterpret_cast<uintptr_t>(d_merges) & 15)) { set_err(err, "%s: d_merges must be 16-byte aligned", what); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

// n <= 1: no launch.  One slot is scanned once and has no neighbour
void linkage_trivial(int64_t n, LinkageCounts* cnt) { cnt->rounds = n; cnt->rowscans = n; }

int linkage_ctx_call(selhip_ctx* c, int measure, int method, double max_height, const selhip_linkage_t* out, int64_t* n_merges_out) {
    if (!c) return SELHIP_E_BADARG;
    const char* const what = "selhip_ctx_linkage";
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", what); return SELHIP_E_STATE; }
    if (!out) { set_err(&c->err, "%s: null selhip_linkage_t (its members may be null, the struct may not)", what); return SELHIP_E_BADARG; }
    if (measure != SELHIP_MEASURE_JACCARD && measure != SELHIP_MEASURE_MAX_CONTAINMENT && measure != SELHIP_MEASURE_SMH_JACCARD) {
        set_err(&c->err, "%s: measure %d is no symmetric similarity (SELHIP_MEASURE_JACCARD, _MAX_CONTAINMENT, _SMH_JACCARD)", what, measure);
        return SELHIP_E_BADARG;
    }
    if (const int rc = linkage_args(&c->err, what, method, max_height, out->d_merges)) return rc;
    const int64_t n = c->n;
    if (n > 0x7FFFFFFFll) { set_err(&c->err, "%s takes up to 2^31 - 1 genomes", what); return SELHIP_E_BADARG; }
    LinkageCounts cnt;
    if (n <= 1) {
        // (the refusals of a matrix call still hold for one genome; none has anything to refuse with no genome)
        if (n == 1) if (const int rc = matrix_call(c, false, measure, SELHIP_F64, 0, 0, nullptr, 0, 0, 0, nullptr, nullptr, T_LINKAGE, what)) return rc;
        linkage_trivial(n, &cnt);
    } else {
        HIPCHK(&c->err, hipSetDevice(c->device));
        DevBlock<double> dist;
        LinkageScratch s;
        hipError_t e = dist.alloc({(size_t)n * (size_t)n});
        if (e == hipSuccess) e = linkage_scratch(&s, n);
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err(&c->err, "%s: %lld x %lld f64 cells of scratch: %s", what, (long long)n, (long long)n, hipGetErrorString(e));
            return SELHIP_E_NOMEM;
        }
        double* const D = dist.part<0>();
        if (const int rc = matrix_call(c, false, measure, SELHIP_F64, 0, n, D, n, n, n, nullptr, nullptr, T_LINKAGE, what)) return rc;
        ClusterBad bad{0, ~0ull};
        int rc;
        {
            TimedCall call(c, T_LINKAGE, false);                                  // (counted by the matrix call above)
            TimerScope t(c, T_LINKAGE);
            hipLaunchKernelGGL(lk_distance_kernel, dim3(grid_for((u64)n * (u64)n, kBlock, 8192)), dim3(kBlock), 0, c->stream, D, (long long)n * n);
            rc = linkage_rounds(&c->err, c->stream, D, n, n, method, max_height, s, &cnt, &bad);
        }
        if (rc) return rc;
        if (bad.count) return linkage_bad_cells(&c->err, what, bad, n);           // (a similarity of +inf: no measure gives one)
        HIPCHK(&c->err, linkage_outputs(c->stream, s, cnt.merges, out->d_merges, out->d_size));
    }
    c->linkage_rounds_last = (int)cnt.rounds;
    c->linkage_merges_last = (int)cnt.merges;
    c->linkage_rowscans_last = (int)std::min<int64_t>(cnt.rowscans, 0x7FFFFFFFll);
    c->linkage_rescans_last = (int)cnt.rescans;
    if (n_merges_out) *n_merges_out = cnt.merges;
    return SELHIP_OK;
}

}  // namespace

// host_gather.hpp -- host side of the winner-takes-all screen (kernel_gather.cuh; include/selection_hip.h section 2m): the checks, the
// scratch and the launches behind selhip_gather and selhip_ctx_gather.
// Part of the kernel translation unit selection_kernels.hip (included there, behind host_nj.hpp); not a stand-alone header.
#pragma once

namespace {

// the survivor tallies / offsets per (query, span), the per-query totals, the segment starts (+ total, + longest segment), the queries' valid masks
using GatherScratch = DevBlock<uint32_t, uint32_t, u64, uint32_t>;
// the candidate entries and their masks: sized from the count launch
using GatherCands = DevBlock<GatherCand, uint32_t>;

// bytes of LDS a workgroup of the current device may stage a segment in: what the device reports, less the pick kernel's own words
int gather_device_lds(int* out) {
    int dev = 0, bytes = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e == hipSuccess) e = hipDeviceGetAttribute(&bytes, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
    if (e != hipSuccess) { (void)hipGetLastError(); return SELHIP_E_HIP; }
    *out = std::max(0, bytes - 1024);
    return SELHIP_OK;
}

template <int WT>
hipError_t gather_launch_pick(hipStream_t st, unsigned grid, size_t dyn, int W, int c_min, int max_picks, const u64* qstart, const GatherCand* cand,
                              const uint32_t* masks, const uint32_t* valid, const GatherOut& o) {
    if (dyn > 48 * 1024) {
        const hipError_t e = hipFuncSetAttribute((const void*)gather_pick_kernel<WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)dyn);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL((gather_pick_kernel<WT>), dim3(grid), dim3(kBlock), dyn, st, W, c_min, max_picks, (long long)(dyn / 4), qstart, cand, masks, valid, o);
    return hipGetLastError();
}

// the arguments every entry checks, before anything touches the device
int gather_check(std::string* err, const char* what, int m, int c_min, int max_picks, const void* d_picks, const void* d_n_picks, const void* d_unexplained) {
    if (m < 1 || m > kGatherMaxM) { set_err(err, "%s: m = %d outside 1 .. %d", what, m, kGatherMaxM); return SELHIP_E_BADARG; }
    if (c_min < 1 || c_min > m) { set_err(err, "%s: c_min = %d outside 1 .. m = %d", what, c_min, m); return SELHIP_E_BADARG; }
    if (max_picks < 1 || max_picks > SELHIP_GATHER_MAX_PICKS) {
        set_err(err, "%s: max_picks = %d outside 1 .. SELHIP_GATHER_MAX_PICKS = %d", what, max_picks, SELHIP_GATHER_MAX_PICKS);
        return SELHIP_E_BADARG;
    }
    if ((reinterpret_cast<uintptr_t>(d_picks) & 15) || (reinterpret_cast<uintptr_t>(d_n_picks) & 3) || (reinterpret_cast<uintptr_t>(d_unexplained) & 3)) {
        set_err(err, "%s: d_picks must be 16-byte aligned, d_n_picks and d_unexplained 4-byte aligned", what);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

// the screen of n_q >= 1 query rows against n_d >= 0 database rows on st; arguments checked (gather_check).  tc: the context whose
// "gather_mask" / "gather_pick" timers the two stages run under, or null; lds_cap: bytes of LDS for a staged segment.  Waits for the
// stream once inside the mask stage and once behind the picks.  The mask kernel is that of matrix_smh_kind(m) -- tile, narrow, wide (m <=
// kGatherMaxM), else generic --; the generic one also takes any base pointer off the 16-byte grid (the others load 16 bytes per lane)
// and, under force_generic ("gather_generic"), every m that is not a tile m.  *kind_out = which
int gather_run(selhip_ctx* tc, std::string* err, const char* what, hipStream_t st, const u64* Q, int64_t n_q, const u64* D, int64_t n_d, int m, int c_min,
               int max_picks, int lds_cap, const GatherOut& o, bool force_generic, int* kind_out) {
    const int W = gather_words(m);
    const bool aligned = !((reinterpret_cast<uintptr_t>(Q) | reinterpret_cast<uintptr_t>(D)) & 15);
    const int kind = !aligned || (force_generic && !matrix_smh_fast(m)) ? kMatrixSmhGeneric : matrix_smh_kind(m);
    *kind_out = kind;
    const MatrixUnits mu = matrix_units(n_q, n_d, kind == kMatrixSmhGeneric ? kWavesPerBlock : matrix_smh_unit_rows(m));
    const long long n_spans = std::max<long long>(mu.n_spans, 1);
    if (mu.n_tiles > 0x7FFFFFFFll) { set_err(err, "%s: too many queries for one launch", what); return SELHIP_E_BADARG; }
    GatherScratch s;
    GatherCands cs;
    hipError_t e = s.alloc({(size_t)n_q * (size_t)n_spans, (size_t)n_q, (size_t)n_q + 2, (size_t)n_q * (size_t)W});
    if (e != hipSuccess) {
        (void)hipGetLastError();
        set_err(err, "%s: scratch for %lld queries x %lld spans: %s", what, (long long)n_q, n_spans, hipGetErrorString(e));
        return SELHIP_E_NOMEM;
    }
    uint32_t* const span_cnt = s.part<0>();
    uint32_t* const qtot = s.part<1>();
    u64* const qstart = s.part<2>();
    uint32_t* const valid = s.part<3>();
    const unsigned grid = (unsigned)std::max<long long>(1, std::min<long long>(mu.n_units, 0x7FFFFFF8ll));
    const unsigned qgrid = grid_for((u64)n_q, 1, 0x7FFFFFFFu);

    // one launch of the mask kernel: the tallies (fill = false) or the entries
    auto mask_launch = [&](bool fill, GatherCand* cand, uint32_t* masks) {
        with_flag(fill, [&](auto F) {
            constexpr bool FILL = decltype(F)::value;
            if (kind == kMatrixSmhGeneric) {
                hipLaunchKernelGGL((gather_mask_generic_kernel<FILL>), dim3(grid), dim3(kBlock), 0, st, Q, D, m, (int)n_q, (int)n_d, (int)mu.n_tiles, mu.n_units,
                                   c_min, n_spans, span_cnt, (const u64*)qstart, cand, masks);
                return;
            }
            if (kind == kMatrixSmhWide) {
                hipLaunchKernelGGL((gather_mask_wide_kernel<FILL>), dim3(grid), dim3(kBlock), 0, st, (const u64x2*)Q, (const u64x2*)D, m / (128 * kMatrixSmhWideNch),
                                   (int)n_q, (int)n_d, (int)mu.n_tiles, mu.n_units, c_min, n_spans, span_cnt, (const u64*)qstart, cand, masks);
                return;
            }
#define SELHIP_GATHER_NARROW_LAUNCH(G) hipLaunchKernelGGL((gather_mask_narrow_kernel<G, FILL>), dim3(grid), dim3(kBlock), 0, st, (const u64x2*)Q, (const u64x2*)D, \
                                                          (int)n_q, (int)n_d, (int)mu.n_tiles, mu.n_units, c_min, n_spans, span_cnt, (const u64*)qstart, cand, masks)
            if (kind == kMatrixSmhNarrow) {
                if (m == 64) SELHIP_GATHER_NARROW_LAUNCH(2);
                else         SELHIP_GATHER_NARROW_LAUNCH(4);
                return;
            }
#undef SELHIP_GATHER_NARROW_LAUNCH
#define SELHIP_GATHER_MASK_LAUNCH(NCH) hipLaunchKernelGGL((gather_mask_kernel<NCH, FILL>), dim3(grid), dim3(kBlock), 0, st, (const u64x2*)Q, (const u64x2*)D, \
                                                          (int)n_q, (int)n_d, (int)mu.n_tiles, mu.n_units, c_min, n_spans, span_cnt, (const u64*)qstart, cand, masks)
            switch (m / 128) {
                case 1:  SELHIP_GATHER_MASK_LAUNCH(1); break;
                case 2:  SELHIP_GATHER_MASK_LAUNCH(2); break;
                case 4:  SELHIP_GATHER_MASK_LAUNCH(4); break;
                default: SELHIP_GATHER_MASK_LAUNCH(8);
            }
#undef SELHIP_GATHER_MASK_LAUNCH
        });
    };
    auto valid_launch = [&]() {
        const unsigned vgrid = grid_for((u64)n_q, kWavesPerBlock, 65536);
#define SELHIP_GATHER_VALID_LAUNCH(NCH) hipLaunchKernelGGL((gather_valid_kernel<NCH>), dim3(vgrid), dim3(kBlock), 0, st, Q, m, (int)n_q, valid)
        if (kind == kMatrixSmhWide) {
            hipLaunchKernelGGL(gather_valid_wide_kernel, dim3(vgrid), dim3(kBlock), 0, st, (const u64x2*)Q, m / (128 * kMatrixSmhWideNch), (int)n_q, valid);
            return;
        }
        if (kind == kMatrixSmhNarrow) {
            if (m == 64) hipLaunchKernelGGL((gather_valid_narrow_kernel<2>), dim3(vgrid), dim3(kBlock), 0, st, (const u64x2*)Q, (int)n_q, valid);
            else         hipLaunchKernelGGL((gather_valid_narrow_kernel<4>), dim3(vgrid), dim3(kBlock), 0, st, (const u64x2*)Q, (int)n_q, valid);
            return;
        }
        switch (kind == kMatrixSmhTile ? m / 128 : 0) {
            case 0:  SELHIP_GATHER_VALID_LAUNCH(0); break;
            case 1:  SELHIP_GATHER_VALID_LAUNCH(1); break;
            case 2:  SELHIP_GATHER_VALID_LAUNCH(2); break;
            case 4:  SELHIP_GATHER_VALID_LAUNCH(4); break;
            default: SELHIP_GATHER_VALID_LAUNCH(8);
        }
#undef SELHIP_GATHER_VALID_LAUNCH
    };

    u64 tail[2] = {0, 0};                                                    // all candidates, the longest segment
    {
        std::optional<TimedCall> call;
        std::optional<TimerScope> t;
        if (tc) { call.emplace(tc, T_GATHER_MASK); t.emplace(tc, T_GATHER_MASK, st); }
        valid_launch();
        if (n_d > 0) {
            mask_launch(false, nullptr, nullptr);
            hipLaunchKernelGGL(gather_scan_rows_kernel, dim3(qgrid), dim3(kBlock), 0, st, span_cnt, n_spans, (int)n_q, qtot);
            hipLaunchKernelGGL(gather_scan_queries_kernel, dim3(1), dim3(kBlock), 0, st, (const uint32_t*)qtot, (int)n_q, qstart);
        } else {
            hipLaunchKernelGGL(gather_clear_kernel, dim3(grid_for((u64)n_q + 2, kBlock, 4096)), dim3(kBlock), 0, st, qstart, (long long)n_q + 2);
        }
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipMemcpyAsync(tail, qstart + n_q, sizeof tail, hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        e = cs.alloc({(size_t)std::max<u64>(tail[0], 1), (size_t)std::max<u64>(tail[0], 1) * (size_t)W});
        if (e != hipSuccess) {
            (void)hipGetLastError();
            set_err(err, "%s: scratch for %llu candidate entries of %d mask words: %s", what, tail[0], W, hipGetErrorString(e));
            return SELHIP_E_NOMEM;
        }
        if (tail[0] > 0) mask_launch(true, cs.part<0>(), cs.part<1>());
        HIPCHK(err, hipGetLastError());
    }
    {
        std::optional<TimedCall> call;
        std::optional<TimerScope> t;
        if (tc) { call.emplace(tc, T_GATHER_PICK); t.emplace(tc, T_GATHER_PICK, st); }
        // LDS for the longest segment, or for as much as the capacity allows (the segments beyond it stream)
        const size_t dyn = (size_t)std::min<u64>((u64)std::max(lds_cap, 0) & ~3ull, tail[1] * (u64)(W + 1) * 4);
        const int wt = W <= 4 ? 4 : W <= 8 ? 8 : W <= 16 ? 16 : W <= 32 ? 32 : 0;
#define SELHIP_GATHER_PICK_LAUNCH(WT) e = gather_launch_pick<WT>(st, qgrid, dyn, W, c_min, max_picks, qstart, cs.part<0>(), cs.part<1>(), valid, o)
        switch (wt) {
            case 4:  SELHIP_GATHER_PICK_LAUNCH(4); break;
            case 8:  SELHIP_GATHER_PICK_LAUNCH(8); break;
            case 16: SELHIP_GATHER_PICK_LAUNCH(16); break;
            case 32: SELHIP_GATHER_PICK_LAUNCH(32); break;
            default: SELHIP_GATHER_PICK_LAUNCH(0);
        }
#undef SELHIP_GATHER_PICK_LAUNCH
        HIPCHK(err, e);
    }
    HIPCHK(err, hipStreamSynchronize(st));
    return SELHIP_OK;
}

int gather_ctx_call(selhip_ctx* c, int c_min, int max_picks, selhip_gather_pick_t* d_picks, int32_t* d_n_picks, int32_t* d_unexplained) {
    if (!c) return SELHIP_E_BADARG;
    const char* const what = "selhip_ctx_gather";
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", what); return SELHIP_E_STATE; }
    if (c->q.n < 0) { set_err(&c->err, "%s: no queries attached (selhip_ctx_upload_queries / _attach_queries)", what); return SELHIP_E_STATE; }
    if (c->m <= 0 || (c->n > 0 && !c->d_aux) || (c->q.n > 0 && !c->q.d_aux)) { set_err(&c->err, "%s before upload/attach of SuperMinHash rows", what); return SELHIP_E_STATE; }
    if (const int rc = gather_check(&c->err, what, c->m, c_min, max_picks, d_picks, d_n_picks, d_unexplained)) return rc;
    if (c->n > 0x7FFFFFFFll || c->q.n > 0x7FFFFFFFll) { set_err(&c->err, "%s takes up to 2^31 - 1 genomes a side", what); return SELHIP_E_BADARG; }
    if (c->q.n == 0) return SELHIP_OK;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int cap = 0;
    if (gather_device_lds(&cap)) { set_err(&c->err, "%s: the device reports no LDS size", what); return SELHIP_E_HIP; }
    if (c->gather_lds_cap > 0) cap = std::min(cap, c->gather_lds_cap);
    return gather_run(c, &c->err, what, c->stream, c->q.d_aux, c->q.n, c->d_aux, c->n, c->m, c_min, max_picks, cap, GatherOut{d_picks, d_n_picks, d_unexplained},
                      c->gather_generic != 0, &c->gather_mask_kernel_used);
}

}  // namespace

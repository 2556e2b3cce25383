// abi_blocks.inc -- building blocks for tests (include/selection_hip.h section 3), synthetic sketches (4), sketch construction (4b),
// device-memory helpers (5) and what the host-only translation units need beyond the public ABI (selhip_internal.h).
// Included by selection_kernels.hip.

extern "C" {

// ---- building blocks -------------------------------------------------------------------------
int selhip_smh_a_pairs(const uint64_t* d_aux, int m, int n_rows, int n_bands,
                       const selhip_int2_t* d_pairs, int64_t n_pairs, uint8_t* d_flags, void* hip_stream) {
    if (!d_aux || !d_pairs || !d_flags || n_pairs < 0 || m <= 0) return SELHIP_E_BADARG;
    if (n_rows <= 0 || n_bands <= 0 || (long long)n_rows * n_bands != m) return SELHIP_E_BADARG;
    if (n_pairs == 0) return SELHIP_OK;
    hipLaunchKernelGGL(pairlist_smh_kernel, dim3((unsigned)((n_pairs + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       (const u64*)d_aux, m, n_rows, n_bands, d_pairs, (long long)n_pairs, (const double*)nullptr, 0.0, 0, 0,
                       d_flags, (selhip_int2_t*)nullptr, (u64)0, (u64*)nullptr);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

int selhip_hll_union_hist(const uint8_t* d_hll, int p, const selhip_int2_t* d_pairs, int64_t n_pairs,
                          uint32_t* d_counts, void* hip_stream) {
    if (!d_hll || !d_pairs || !d_counts || n_pairs < 0 || p < 4 || p > 20) return SELHIP_E_BADARG;
    if (n_pairs == 0) return SELHIP_OK;
    hipLaunchKernelGGL(hll_union_hist_kernel, dim3(grid_for((u64)n_pairs, kWavesPerBlock, 4096)), dim3(kBlock), 0,
                       (hipStream_t)hip_stream, d_hll, p, d_pairs, (const u64*)nullptr, (u64)n_pairs, (u64)n_pairs, d_counts);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

int selhip_hll_bitslice(const uint8_t* d_hll, int64_t n, uint32_t* d_planes, uint8_t* d_gmax, int* khi_out, void* hip_stream) {
    if (!d_hll || !d_planes || !d_gmax || !khi_out || n < 0) return SELHIP_E_BADARG;
    *khi_out = 1;
    if (n == 0) return SELHIP_OK;
    int* d_max = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&d_max, sizeof(int)));
    const int rc = build_bitslices(nullptr, (hipStream_t)hip_stream, d_hll, n, d_planes, d_gmax, d_max, khi_out);
    (void)hipFree(d_max);
    return rc;
}

int selhip_hll_union_hist_planes(const uint32_t* d_planes, const uint8_t* d_gmax, int khi, const selhip_int2_t* d_pairs, int64_t n_pairs,
                                 uint32_t* d_counts, void* hip_stream) {
    if (!d_planes || !d_gmax || !d_pairs || !d_counts || n_pairs < 0 || khi < 1 || khi > 64) return SELHIP_E_BADARG;
    if (n_pairs == 0) return SELHIP_OK;
    u64* d_n = nullptr;
    HIPCHK(nullptr, hipMalloc((void**)&d_n, sizeof(u64)));
    const u64 np = (u64)n_pairs;
    hipError_t e = hipMemcpyAsync(d_n, &np, sizeof(u64), hipMemcpyHostToDevice, (hipStream_t)hip_stream);
    if (e == hipSuccess) e = launch_hist_bs(khi, 2048, (hipStream_t)hip_stream, d_planes, d_gmax, d_pairs, d_n, np, d_counts, 0, ~0ull, 1, ~0ull);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)hip_stream);
    (void)hipFree(d_n);
    HIPCHK(nullptr, e);
    return SELHIP_OK;
}

int selhip_ertl_estimate(const uint32_t* d_counts, int64_t n, int p, int fp_mode, double* d_est, void* hip_stream) {
    if (!d_counts || !d_est || n < 0 || p < 4 || p > 20) return SELHIP_E_BADARG;
    if (n == 0) return SELHIP_OK;
    HIPCHK(nullptr, launch_select<0>(fp_mode == SELHIP_FP_FMA, (hipStream_t)hip_stream, grid_for((u64)n, kWave, 8192), d_counts,
                                     nullptr, (u64)n, (u64)n, p, d_est, nullptr, nullptr, 0.0, nullptr, 0, nullptr, nullptr, nullptr));
    return SELHIP_OK;
}

int selhip_smh_match_counts(const uint64_t* d_aux, int m, const selhip_int2_t* d_pairs, int64_t n_pairs,
                            int32_t* d_matches, void* hip_stream) {
    if (!d_aux || !d_pairs || !d_matches || n_pairs < 0 || m <= 0) return SELHIP_E_BADARG;
    if (n_pairs == 0) return SELHIP_OK;
    const long long threads = (long long)n_pairs * kWave;
    hipLaunchKernelGGL(match_count_kernel, dim3((unsigned)((threads + kBlock - 1) / kBlock)), dim3(kBlock), 0, (hipStream_t)hip_stream,
                       (const u64*)d_aux, m, d_pairs, (long long)n_pairs, d_matches);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

int selhip_hll_fold(const uint8_t* d_hll, int64_t n, int p, int p_aux, uint8_t* d_out, void* hip_stream) {
    if (n < 0 || p < 4 || p > 20 || p_aux < 4 || p_aux > p || p_aux > kMaxAuxP) {
        set_err(nullptr, "selhip_hll_fold: p %d, p_aux %d: need 4 <= p <= 20 and 4 <= p_aux <= min(p, %d)", p, p_aux, kMaxAuxP);
        return SELHIP_E_BADARG;
    }
    if (n == 0) return SELHIP_OK;
    if (!d_hll || !d_out) { set_err(nullptr, "selhip_hll_fold: null pointer"); return SELHIP_E_BADARG; }
    if (((uintptr_t)d_hll & 15) || ((uintptr_t)d_out & 15)) { set_err(nullptr, "selhip_hll_fold: pointers must be 16-byte aligned"); return SELHIP_E_BADARG; }
    HIPCHK(nullptr, launch_hll_fold((hipStream_t)hip_stream, d_hll, (u64)n, p, p_aux, d_out));
    return SELHIP_OK;
}

// (selhip_multi_select lives in selhip_multi.hip, selhip_ooc_select in selhip_ooc.hip: host-only translation units of this library
// built on the context API above; what they need beyond it is declared in selhip_internal.h and defined here)
void selhip_internal_set_error(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

int selhip_internal_reserve_replica(selhip_ctx* c, int64_t rows_padded, int m, int p_hll, int p_aux,
                                    uint8_t** d_hll, uint64_t** d_aux, double** d_cards, uint8_t** d_aux_hll) {
    if (!c || rows_padded < 0 || m <= 0 || p_hll < 4 || p_hll > 20 || !d_hll || !d_aux || !d_cards) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    const size_t rows = (size_t)std::max<int64_t>(rows_padded, 1);
    HIPCHK(&c->err, c->own_hll.ensure(rows << p_hll));
    HIPCHK(&c->err, c->own_aux.ensure(rows * (size_t)m));
    HIPCHK(&c->err, c->own_cards.ensure(rows));
    *d_hll = c->own_hll.p; *d_aux = (uint64_t*)c->own_aux.p; *d_cards = c->own_cards.p;
    if (p_aux > 0) {
        if (!d_aux_hll || p_aux > kMaxAuxP) return SELHIP_E_BADARG;
        HIPCHK(&c->err, c->own_aux_hll.ensure(rows << p_aux));
        *d_aux_hll = c->own_aux_hll.p;
    }
    return SELHIP_OK;
}

void* selhip_internal_stream(selhip_ctx* c) { return c ? (void*)c->stream : nullptr; }

// ---- synthetic data ----------------------------------------------------------------------------
int selhip_synth_generate(const selhip_synth_t* sp_in, int64_t g_begin, int64_t g_end,
                          uint8_t* d_hll, uint64_t* d_aux, uint8_t* d_aux_hll, void* hip_stream) {
    if (!sp_in || !d_hll || !d_aux || g_begin < 0 || g_end < g_begin) return SELHIP_E_BADARG;
    if (!is_pow2(sp_in->m) || sp_in->m > 4096 || sp_in->cluster_size < 1 || sp_in->p_aux < 0 || sp_in->p_aux > 12) return SELHIP_E_BADARG;
    if (g_end == g_begin) return SELHIP_OK;
    selhip::SynthParams sp;
    sp.seed = sp_in->seed; sp.n_genomes = sp_in->n_genomes; sp.m = sp_in->m; sp.p_aux = sp_in->p_aux;
    sp.cluster_size = sp_in->cluster_size; sp.mode = sp_in->mode; sp.n_sh_lo = sp_in->n_sh_lo; sp.n_sh_hi = sp_in->n_sh_hi;
    const size_t smem = (size_t)sp.m * 8 + 16384 * 4 + (sp.p_aux ? ((size_t)4 << sp.p_aux) : 0);
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] { attr_err = hipFuncSetAttribute((const void*)synth_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    HIPCHK(nullptr, attr_err);
    hipLaunchKernelGGL(synth_kernel, dim3((unsigned)(g_end - g_begin)), dim3(kBlock), smem, (hipStream_t)hip_stream,
                       sp, (long long)g_begin, (long long)g_end, d_hll, (u64*)d_aux, d_aux_hll);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}


int selhip_build_sketches(const uint8_t* d_codes, const int64_t* d_offsets, int64_t n_genomes, int k, int m, int p_aux,
                          uint8_t* d_hll, uint64_t* d_smh, uint8_t* d_aux_hll, void* hip_stream) {
    if (!d_codes || !d_offsets || !d_hll || n_genomes < 0 || k < 1 || k > 32) { set_err(nullptr, "bad argument"); return SELHIP_E_BADARG; }
    if (d_smh && (!is_pow2(m) || m > 2048)) { set_err(nullptr, "m must be a power of two <= 2048 (SizePow2Policy rounds up: pass the rounded value)"); return SELHIP_E_BADARG; }
    if (d_aux_hll && (p_aux < 4 || p_aux > 12)) { set_err(nullptr, "p_aux out of range [4,12]"); return SELHIP_E_BADARG; }
    if (n_genomes == 0) return SELHIP_OK;
    const size_t ms = d_smh ? (size_t)m : 0;
    const size_t smem = ms * 8 + 16384 + (d_aux_hll ? ((((size_t)1 << p_aux) + 3) / 4 * 4) : 0) + ms * 12 + 16;
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] { attr_err = hipFuncSetAttribute((const void*)sketch_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    HIPCHK(nullptr, attr_err);
    // one block per genome; few genomes: 16 waves per block, so that a CU that holds a single block still has 4 waves per SIMD
    const unsigned threads = n_genomes < 2048 ? 1024u : (unsigned)kBlock;
    hipLaunchKernelGGL(sketch_build_kernel, dim3((unsigned)n_genomes), dim3(threads), smem, (hipStream_t)hip_stream,
                       d_codes, (const long long*)d_offsets, k, m, p_aux, d_hll, (u64*)d_smh, d_aux_hll);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

#ifdef SELHIP_JOIN_TRACE
int selhip_debug_join_trace(unsigned long long* h_out, int clear) {        // development build only (scripts/join_trace.py)
    if (clear) {
        void* p = nullptr;
        HIPCHK(nullptr, hipGetSymbolAddress(&p, HIP_SYMBOL(g_join_trace)));
        HIPCHK(nullptr, hipMemset(p, 0, sizeof(unsigned long long) * 4 * (1 << 17)));
        return SELHIP_OK;
    }
    HIPCHK(nullptr, hipMemcpyFromSymbol(h_out, HIP_SYMBOL(g_join_trace), sizeof(unsigned long long) * 4 * (1 << 17)));
    return SELHIP_OK;
}
#endif

int selhip_malloc(void** d_ptr, size_t bytes) {
    if (!d_ptr) return SELHIP_E_BADARG;
    HIPCHK(nullptr, hipMalloc(d_ptr, bytes ? bytes : 1));
    return SELHIP_OK;
}
int selhip_free(void* d_ptr) {
    if (d_ptr) HIPCHK(nullptr, hipFree(d_ptr));
    return SELHIP_OK;
}
int selhip_memcpy_h2d(void* d_dst, const void* h_src, size_t bytes) {
    if (bytes) HIPCHK(nullptr, hipMemcpy(d_dst, h_src, bytes, hipMemcpyHostToDevice));
    return SELHIP_OK;
}
int selhip_memcpy_d2h(void* h_dst, const void* d_src, size_t bytes) {
    if (bytes) HIPCHK(nullptr, hipMemcpy(h_dst, d_src, bytes, hipMemcpyDeviceToHost));
    return SELHIP_OK;
}
int selhip_device_synchronize(void) {
    HIPCHK(nullptr, hipDeviceSynchronize());
    return SELHIP_OK;
}

int selhip_permute_rows(const void* d_src, void* d_dst, const int32_t* d_perm, int64_t n_rows,
                        int64_t row_bytes, void* hip_stream) {
    if (!d_src || !d_dst || !d_perm || n_rows < 0 || row_bytes <= 0) return SELHIP_E_BADARG;
    if (n_rows == 0) return SELHIP_OK;
    const unsigned grid = (unsigned)std::min<int64_t>(n_rows, 65536);
    if (row_bytes % 16 == 0 && !((uintptr_t)d_src & 15) && !((uintptr_t)d_dst & 15))
        hipLaunchKernelGGL(permute_rows_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)hip_stream,
                           (const uint4*)d_src, (uint4*)d_dst, d_perm, (long long)n_rows, (long long)(row_bytes / 16));
    else
        hipLaunchKernelGGL(permute_bytes_kernel, dim3(grid), dim3(kBlock), 0, (hipStream_t)hip_stream,
                           (const uint8_t*)d_src, (uint8_t*)d_dst, d_perm, (long long)n_rows, (long long)row_bytes);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

}  // extern "C"

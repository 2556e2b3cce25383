// abi_compat.inc -- the drop-in launchers launch_kernel_smh / launch_kernel_CBsmh (+ 64-bit twins) with the parameter lists of the
// reference's src/selection_kernels_wrapper.hpp:11-45.  Included by selection_kernels.hip.


namespace {
struct CompatWs {
    std::mutex mu;
    DevBuf<selhip_int2_t> surv;
    DevBuf<uint32_t> counts;
    DevBuf<u64> surv_count;
    selhip_ctx* ctx[64] = {};          // implicit-enumeration path: one cached context per device (process lifetime)
};
CompatWs g_ws;
constexpr long long kCompatChunk = 1ll << 20;      // explicit pair lists are processed this many pairs at a time (256 MiB of histograms)

// select for the drop-in launchers: the reference signature carries no genome count, so the truncated
// cardinalities are taken on the fly from cards[rank]; output record = struct Result {x, y, (float)J}.
template <bool FMA, typename CountT>
__global__ __launch_bounds__(kWave)
void compat_select_kernel(const uint32_t* __restrict__ counts, const u64* __restrict__ n_dev, u64 cap, int p,
                          double relerr_scaled, const selhip_int2_t* __restrict__ pairs,
                          const double* __restrict__ cards, double tau,
                          selhip_result_t* __restrict__ out, CountT* __restrict__ out_count) {
    __shared__ uint32_t lds[64 * 65];
    const int lane = threadIdx.x;
    u64 n = *n_dev;
    if (n > cap) n = cap;
    for (u64 base = (u64)blockIdx.x * kWave; base < n; base += (u64)gridDim.x * kWave) {
        __syncthreads();
        for (int r = 0; r < kWave; ++r) {
            u64 j = base + r;
            lds[lane * 65 + r] = (j < n) ? counts[j * 64 + lane] : (lane == 0 ? (1u << p) : 0u);
        }
        __syncthreads();
        const u64 j = base + lane;
        LdsCounts c{lds + lane};
        double t = selhip::ertl_ml_estimate<FMA>(c, (unsigned)p, (unsigned)(64 - p), relerr_scaled);
        if (j < n) {
            const selhip_int2_t pr = pairs[j];
            const double e1 = (double)selhip::trunc_card(cards[pr.x]), e2 = (double)selhip::trunc_card(cards[pr.y]);
            const double jacc = (e1 + e2 - t) / t;                           // selection.cpp:287
            if (jacc >= tau) {                                               // selection.cpp:288
                const CountT idx = atomicAdd(out_count, (CountT)1);
                out[idx].x = pr.x; out[idx].y = pr.y; out[idx].sim = (float)jacc;
            }
        }
    }
}

// implicit enumeration: the context's result records {i, k, double J} -> struct Result {x, y, (float)J}, and the count
template <typename CountT>
__global__ __launch_bounds__(kBlock)
void compat_convert_kernel(const selhip_pair_t* __restrict__ res, u64 n, selhip_result_t* __restrict__ out, CountT* __restrict__ out_count) {
    for (u64 j = (u64)blockIdx.x * kBlock + threadIdx.x; j < n; j += (u64)gridDim.x * kBlock) {
        const selhip_pair_t r = res[j];
        out[j].x = r.i; out[j].y = r.k; out[j].sim = (float)r.jaccard;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) *out_count = (CountT)n;
}

template <typename CountT>
int compat_launch(bool use_cb, const uint8_t* main_sketches, const uint64_t* aux, const double* cards,
                  const selhip_int2_t* pairs, long long total_pairs, double tau, int m_aux, int m_hll,
                  int n_rows, int n_bands, selhip_result_t* out, CountT* out_count) {
    if (!main_sketches || !aux || !cards || !out || !out_count) { set_err(nullptr, "null pointer argument"); return SELHIP_E_BADARG; }
    if (total_pairs < 0 || m_aux <= 0 || !is_pow2(m_hll) || m_hll < 16) { set_err(nullptr, "bad sizes"); return SELHIP_E_BADARG; }
    if (n_rows <= 0 || n_bands <= 0 || (long long)n_rows * n_bands != m_aux) { set_err(nullptr, "n_rows*n_bands != m_aux"); return SELHIP_E_BADARG; }
    hipStream_t st = nullptr;                                        // default stream, like the reference
    HIPCHK(nullptr, hipMemsetAsync(out_count, 0, sizeof(CountT), st));  // selection_kernels.cu:137,166
    if (total_pairs == 0) return SELHIP_OK;
    if (pairs && ((uintptr_t)pairs & 7)) { set_err(nullptr, "the pair list must be 8-byte aligned (an array of int2)"); return SELHIP_E_BADARG; }
    const int p = ilog2(m_hll);
    std::lock_guard<std::mutex> lk(g_ws.mu);
    if (!pairs) {
        // pairs == NULL: the list is the implicit triangle i < k < n of the reference driver (selection_cuda.cpp:146-150), which is
        // never materialised -- total_pairs must be n(n-1)/2 and fixes n.  Runs through a cached context attached to the caller's
        // device arrays (all-pairs signature join + stage 2); this variant waits for the pass before it returns.
        const long long nn = (long long)((1.0 + std::sqrt(1.0 + 8.0 * (double)total_pairs)) / 2.0);
        long long n = nn;
        for (long long c = nn - 1; c <= nn + 1; ++c) if (c >= 2 && c * (c - 1) / 2 == total_pairs) n = c;
        if (n < 2 || n * (n - 1) / 2 != total_pairs) { set_err(nullptr, "pairs == NULL needs total_pairs = n(n-1)/2 (the whole triangle); got %lld", total_pairs); return SELHIP_E_BADARG; }
        int dev = 0;
        HIPCHK(nullptr, hipGetDevice(&dev));
        if (dev < 0 || dev >= 64) { set_err(nullptr, "device index out of range"); return SELHIP_E_BADARG; }
        if (!g_ws.ctx[dev]) { int r = selhip_ctx_create(&g_ws.ctx[dev], dev); if (r) return r; }
        selhip_ctx* c = g_ws.ctx[dev];
        int r = selhip_ctx_attach(c, main_sketches, aux, cards, n, m_aux, p);
        if (!r) r = selhip_ctx_run(c, use_cb ? SELHIP_MODE_CB_SMH : SELHIP_MODE_SMH, SELHIP_ALGO_AUTO, (float)tau, n_rows, n_bands, 0, n);
        if (r) { set_err(nullptr, "%s", selhip_last_error(c)); return r; }
        const u64 cnt = c->last.n_results;
        if (sizeof(CountT) == 4 && cnt > 0x7FFFFFFFull) { set_err(nullptr, "more than 2^31 selected pairs: use the 64-bit launcher"); return SELHIP_E_OVERFLOW; }
        hipLaunchKernelGGL((compat_convert_kernel<CountT>), dim3(grid_for(cnt, kBlock, 4096)), dim3(kBlock), 0, c->stream, c->results.p, cnt, out, out_count);
        HIPCHK(nullptr, hipGetLastError());
        return SELHIP_OK;
    }
    const long long chunk = std::min(total_pairs, kCompatChunk);
    HIPCHK(nullptr, g_ws.surv.ensure((size_t)chunk));
    HIPCHK(nullptr, g_ws.counts.ensure((size_t)chunk * 64));
    HIPCHK(nullptr, g_ws.surv_count.ensure(1));
    for (long long off = 0; off < total_pairs; off += chunk) {
        const long long len = std::min(chunk, total_pairs - off);
        HIPCHK(nullptr, hipMemsetAsync(g_ws.surv_count.p, 0, sizeof(u64), st));
        // stage 1: pairs_direct_kernel in its launcher form (kernel_pairs.cuh) -- 16 lanes per pair on contiguous 128-byte pieces of both
        // rows, one append per block and batch (it replaced the lane-per-pair pairlist_smh_kernel here)
        const PairsDirectShape sh = pairs_direct_shape((u64)len);
        hipLaunchKernelGGL(pairs_direct_kernel<true>, dim3(sh.grid), dim3(kPairsBlock), 0, st,
                           (const u64*)aux, m_aux, n_rows, n_bands, pairs + off, (u64)len, 0, (const u64*)nullptr, cards, tau, use_cb ? 1 : 0, sh.gpw,
                           g_ws.surv.p, (u64)g_ws.surv.cap, g_ws.surv_count.p, (PassCounters*)nullptr);
        HIPCHK(nullptr, hipGetLastError());
        hipLaunchKernelGGL(hll_union_hist_kernel, dim3(2048), dim3(kBlock), 0, st, main_sketches, p, g_ws.surv.p,
                           g_ws.surv_count.p, (u64)0, (u64)g_ws.surv.cap, g_ws.counts.p);
        HIPCHK(nullptr, hipGetLastError());
        hipLaunchKernelGGL((compat_select_kernel<true, CountT>), dim3(4096), dim3(kWave), 0, st,
                           g_ws.counts.p, g_ws.surv_count.p, (u64)g_ws.surv.cap, p, relerr_scaled_for(p), g_ws.surv.p,
                           cards, tau, out, out_count);
        HIPCHK(nullptr, hipGetLastError());
    }
    return SELHIP_OK;
}
}  // namespace

extern "C" {

int launch_kernel_smh(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                      const selhip_int2_t* pairs, int total_pairs, double tau,
                      int m_aux, int m_hll, int n_rows, int n_bands,
                      selhip_result_t* out, int* out_count, int blockSize) {
    (void)blockSize;
    return compat_launch<int>(false, main_sketches, aux_sketches, cards, pairs, total_pairs, tau, m_aux, m_hll, n_rows, n_bands, out, out_count);
}

int launch_kernel_CBsmh(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                        const selhip_int2_t* pairs, int total_pairs, double tau,
                        int m_aux, int m_hll, int n_rows, int n_bands,
                        selhip_result_t* out, int* out_count, int blockSize) {
    (void)blockSize;
    return compat_launch<int>(true, main_sketches, aux_sketches, cards, pairs, total_pairs, tau, m_aux, m_hll, n_rows, n_bands, out, out_count);
}

// 64-bit variants: the reference's `int total_pairs` / `int idx` (selection_kernels.cu:29-30) overflow beyond 2^31 pairs
// (N > 65 536 genomes); same parameter lists with int64_t total_pairs and a 64-bit *out_count.
int launch_kernel_smh64(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                        const selhip_int2_t* pairs, int64_t total_pairs, double tau,
                        int m_aux, int m_hll, int n_rows, int n_bands,
                        selhip_result_t* out, int64_t* out_count, int blockSize) {
    (void)blockSize;
    return compat_launch<unsigned long long>(false, main_sketches, aux_sketches, cards, pairs, total_pairs, tau, m_aux, m_hll, n_rows, n_bands, out,
                                             reinterpret_cast<unsigned long long*>(out_count));
}

int launch_kernel_CBsmh64(const uint8_t* main_sketches, const uint64_t* aux_sketches, const double* cards,
                          const selhip_int2_t* pairs, int64_t total_pairs, double tau,
                          int m_aux, int m_hll, int n_rows, int n_bands,
                          selhip_result_t* out, int64_t* out_count, int blockSize) {
    (void)blockSize;
    return compat_launch<unsigned long long>(true, main_sketches, aux_sketches, cards, pairs, total_pairs, tau, m_aux, m_hll, n_rows, n_bands, out,
                                             reinterpret_cast<unsigned long long*>(out_count));
}

}  // extern "C"

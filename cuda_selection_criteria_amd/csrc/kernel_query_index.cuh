// kernel_query_index.cuh -- ALGO_INDEX of the query passes: stage 1 as a lookup in a sorted band-signature index of the database.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
//
// The index (built once per database and band shape, host_query.hpp: build_query_index): for every band b the n_d 32-bit band
// signatures of the database sorted ascending, idx_sig[b * n_d + j], with the database ranks they belong to, idx_rank[b * n_d + j].
// The sort (sigkey_build_kernel -> rocprim::radix_sort_pairs on (band << 32) | signature) is stable and the ranks go in ascending, so
// inside a run of equal signatures the ranks ascend.  On top of each band's segment sits a bucket directory, idx_dir[b][v] = the first
// entry whose signature's top dir_bits bits are >= v (2^dir_bits + 1 offsets per band, one per two to four entries): two adjacent
// directory words bound a search to the few entries of one bucket.  9 to 10 bytes per (genome, band); every offset into it is 64-bit.
//   query_index_pack_kernel    the sorted 64-bit keys down to the 32-bit signatures the probe reads
//   query_index_dir_kernel     the bucket directory, one binary search per directory word
//   query_index_probe_kernel   one lane per (query, band), a wave per (band, 64 queries): the run of the query's band signature in the band's sorted segment; every
//                              database genome of the run inside the query's window is appended to the candidate list iff the band is
//                              the FIRST whose 32-bit signatures are equal -- so a pair with any equal band is appended exactly once:
//                              the list query_sig_join_kernel writes (in another order), counted in n_pre like that one
#pragma once

namespace {

__global__ __launch_bounds__(kBlock)
void query_index_pack_kernel(const u64* __restrict__ keys, long long total, uint32_t* __restrict__ idx_sig) {
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < total; t += (long long)gridDim.x * kBlock) idx_sig[t] = (uint32_t)keys[t];
}

// directory words per band
__host__ __device__ __forceinline__ long long query_index_dir_stride(int dir_bits) { return (1ll << dir_bits) + 1; }

__global__ __launch_bounds__(kBlock)
void query_index_dir_kernel(const uint32_t* __restrict__ idx_sig, int n_d, int nb, int dir_bits, int* __restrict__ idx_dir) {
    const long long stride = query_index_dir_stride(dir_bits), total = stride * nb;
    for (long long t = (long long)blockIdx.x * kBlock + threadIdx.x; t < total; t += (long long)gridDim.x * kBlock) {
        const int b = (int)(t / stride);
        const long long v = t - (long long)b * stride;
        int lo = 0, hi = n_d;
        if (v == stride - 1) lo = n_d;
        else if (v > 0) {                                                 // (v = 0: offset 0; dir_bits >= 1 here)
            const uint32_t key = (uint32_t)v << (32 - dir_bits);
            const uint32_t* seg = idx_sig + (long long)b * n_d;
            while (lo < hi) {
                const int mid = lo + (hi - lo) / 2;
                if (seg[mid] >= key) hi = mid; else lo = mid + 1;
            }
        }
        idx_dir[t] = lo;
    }
}

// (q, d) with an equal signature in band b: taken iff d lies in q's window and no earlier band is equal as well
__device__ __forceinline__ bool query_index_take(const uint32_t* __restrict__ sig_q, const uint32_t* __restrict__ sig_d, int nb, int q, int d,
                                                 int b, int lo_q, int hi_q) {
    if (d < lo_q || d > hi_q) return false;
    // the bands before b, four per 16-byte load (rows are n_bands dwords, n_bands a multiple of 8)
    const uint4* x = reinterpret_cast<const uint4*>(sig_q + (size_t)q * nb);
    const uint4* y = reinterpret_cast<const uint4*>(sig_d + (size_t)d * nb);
    const int full = b >> 2, rest = b & 3;
    for (int g = 0; g < full; ++g) {
        const uint4 u = x[g], v = y[g];
        if (u.x == v.x || u.y == v.y || u.z == v.z || u.w == v.w) return false;
    }
    if (rest) {                                                           // (b < n_bands: group `full` lies inside the rows)
        const uint4 u = x[full], v = y[full];
        if (u.x == v.x || (rest > 1 && u.y == v.y) || (rest > 2 && u.z == v.z)) return false;
    }
    return true;
}

// ---------------------------------------------------------------------------------------------
// query_index_probe_kernel.  A wave takes 64 consecutive queries of ONE band (work item = (band, group of 64 queries), band-major), so
// the band, the segment base and the trip count of the first-band test are wave-uniform, and the first levels of the lanes' searches
// read the same lines.  A lane takes the bounds of its key's bucket from the directory (idx_dir == nullptr: the whole segment) and
// searches the lower and the upper bound of the key inside them together (two independent loads per level, one dependent chain) ->
// its run [s, s + len).  Whatever the signatures' distribution the search is exact: a crowded bucket only costs more levels, up to
// the ~log2(n_d) of the plain search.  A query with an empty window searches nothing.
// A wave whose longest run is <= 1 lets every lane test its own entry.  Otherwise (clustered, near-duplicate or identical genomes:
// runs up to n_d) the wave's 64 runs are laid end to end by a wave prefix sum kept in LDS, and the 64 lanes take 64 consecutive
// entries of that sequence per step, each finding its owner run by a 6-level search of the prefix sums -- so a long run costs
// len / 64 steps of the whole wave, not len steps of one lane.
// Not built: cutting the window out of a run by two more searches on the ascending ranks (the long-run test
// does not need it: an entry outside the window costs one rank load); a k-ary pivot layout (with the directory the searches are
// ~2 us of the kernel's ~20).
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock)
void query_index_probe_kernel(const uint32_t* __restrict__ sig_q, const uint32_t* __restrict__ sig_d, const uint32_t* __restrict__ idx_sig,
                              const int* __restrict__ idx_rank, const int* __restrict__ idx_dir, int dir_bits, int n_q, int n_d, int nb,
                              const int* __restrict__ lo, const int* __restrict__ hi, selhip_int2_t* __restrict__ cand, u64 cand_cap,
                              PassCounters* __restrict__ pc) {
    __shared__ selhip_int2_t app_lds[kWavesPerBlock * kAppendCap];
    __shared__ u64 run_off[kWavesPerBlock][kWave];          // exclusive prefix sums of the wave's run lengths
    __shared__ int run_at[kWavesPerBlock][kWave];           // where each run starts in the band's segment
    __shared__ int run_lo[kWavesPerBlock][kWave], run_hi[kWavesPerBlock][kWave];     // its query's window
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const long long groups = ((long long)n_q + kWave - 1) / kWave, n_items = groups * nb;
    WaveAppender app;
    app.init(app_lds, wave, cand, cand_cap, &pc->n_pre);
    for (long long w = (long long)blockIdx.x * kWavesPerBlock + wave; w < n_items; w += (long long)gridDim.x * kWavesPerBlock) {   // wave-uniform
        const int b = (int)(w / groups);
        const int q0 = (int)((w - (long long)b * groups) * kWave);
        const int q = q0 + lane;
        int lo_q = 0, hi_q = -1;
        if (q < n_q) { lo_q = lo[q]; hi_q = hi[q]; }
        const uint32_t* seg = idx_sig + (long long)b * n_d;
        const int* seg_rank = idx_rank + (long long)b * n_d;
        int s = 0, len = 0;
        if (hi_q >= lo_q) {
            const uint32_t key = sig_q[(size_t)q * nb + b];
            // a1 = first entry >= key, a2 = first entry > key
            int a1 = 0, b1 = n_d;
            if (idx_dir) {
                const int* dw = idx_dir + (long long)b * query_index_dir_stride(dir_bits) + (dir_bits ? key >> (32 - dir_bits) : 0u);
                a1 = dw[0]; b1 = dw[1];
            }
            int a2 = a1, b2 = b1;
            while (a1 < b1 || a2 < b2) {
                const int m1 = a1 + (b1 - a1) / 2, m2 = a2 + (b2 - a2) / 2;
                const uint32_t v1 = seg[min(m1, n_d - 1)], v2 = seg[min(m2, n_d - 1)];
                if (a1 < b1) { if (v1 >= key) b1 = m1; else a1 = m1 + 1; }
                if (a2 < b2) { if (v2 > key) b2 = m2; else a2 = m2 + 1; }
            }
            s = a1;
            len = a2 - a1;
        }
        if (__ballot(len > 1) == 0) {
            int d = 0;
            bool take = false;
            if (len == 1) {
                d = seg_rank[s];
                take = query_index_take(sig_q, sig_d, nb, q, d, b, lo_q, hi_q);
            }
            app.push(take, q, d, lane);
            continue;
        }
        u64 incl = (u64)len;
#pragma unroll
        for (int sft = 1; sft < kWave; sft <<= 1) {
            const u64 up = __shfl_up(incl, sft, kWave);
            if (lane >= sft) incl += up;
        }
        const u64 total = __shfl(incl, kWave - 1, kWave);
        run_off[wave][lane] = incl - (u64)len;
        run_at[wave][lane] = s;
        run_lo[wave][lane] = lo_q; run_hi[wave][lane] = hi_q;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (u64 f0 = 0; f0 < total; f0 += kWave) {                                            // wave-uniform trip count
            const u64 f = f0 + lane;
            int d = 0, o = 0;                                                                   // o: the last run that starts at or before f
            bool take = false;
            if (f < total) {
#pragma unroll
                for (int sft = kWave / 2; sft > 0; sft >>= 1)
                    if (run_off[wave][o + sft] <= f) o += sft;
                d = seg_rank[run_at[wave][o] + (int)(f - run_off[wave][o])];
                take = query_index_take(sig_q, sig_d, nb, q0 + o, d, b, run_lo[wave][o], run_hi[wave][o]);
            }
            app.push(take, q0 + o, d, lane);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");                                 // the next round rewrites the run arrays
    }
    app.flush(lane);
}

}  // namespace

// kernel_mcl.cuh -- Markov clustering (van Dongen's MCL) of a symmetric CSR similarity graph, on the device (include/selection_hip.h
// section 2o, THE DEFINITION; host side in host_mcl.hpp).  Part of libselhip.so; included by selection_kernels.hip only, behind
// kernel_graph.cuh (ClusterBad, graph_image, the union-find the final labels go through) and kernel_adjacency.cuh (adj_init_kernel).
//
// The flow matrix lives in an ELL layout: K = max_entries slots per column, row[n * K] int32 ascending inside a column, val[n * K] f64,
// cnt[n] entries in use.  Two such buffers alternate; nothing is allocated and nothing is counted ahead inside the loop, because a
// column never holds more than K entries and so never gathers more than K * K products.
//   mcl_check_kernel      every value finite and >= 0, every column in [0, n), every row offset in order: tallied, nothing written
//   mcl_start_kernel      CSR row j -> column j: the self loop, the K best, the normalisation; one workgroup per row.  Rows of up to
//                         4 095 entries are staged in LDS and ordered there; a longer row is selected in K rounds of two passes
//                         over global memory each -- for correctness only, no graph of the passes has such rows in numbers
//   mcl_step_kernel<C>    one whole iteration of one column: expansion, inflation, pruning, cut, normalisation, chaos
//     C = 0  K <= 8    one wave per column, at most 64 products, one per lane: keys and values in registers, both orderings are the
//                      21-step network of kernel_adjacency.cuh over cross-lane moves; no LDS, no barrier, four columns per block
//     C = 1  K <= 32   one workgroup of 256 per column, at most 1 024 products: 12 B each in LDS (14 092 B with the column's own arrays)
//     C = 2  K <= 64   one workgroup of 512 per column, at most 4 096 products: 12 B each in LDS (50 956 B), inside the 64 KiB a
//                      workgroup may take
// A column's work.  Its c <= K entries (k_s, w_s) name the source columns; product p of the column is entry t of source s and gets the
// key (row i << 12 | s << 6 | t).  The keys are SORTED rather than merged K ways: the sort is the one network the project already
// trusts, its cost follows the products actually there (n = 2^ceil(log2 P), and P falls fast as the flow converges), and the key order
// (i, s) is exactly the order the definition adds in, so the lane at the head of a run of equal i walks its run -- at most K products,
// each multiplied on its own (__dmul_rn) and added in ascending s (__dadd_rn) -- and no sum depends on how the lanes were scheduled.
// A K-way merge would need a serial cursor per source or a search per (row, source).  The products themselves are not staged: a key
// names its source entry, and the head reads the 8-byte value again from the (L2-resident) input column.
// Behind the sums the same 12 bytes hold (bits of the inflated value, row): positive doubles order like their bits, so the second
// ordering -- value descending, row ascending, pruned and non-head slots as zeros behind -- leaves the K best at the front.  Wave 0
// ranks them by row (K * K reads of LDS), adds them in ascending row order, divides, and writes the column and its chaos.
// The matrix chaos is an atomic maximum over the order-preserving integer image of kernel_graph.cuh: no floating-point atomic anywhere,
// and no lane waits for another workgroup.  With r == 2.0 every output is a function of the input alone, bit for bit.
#pragma once

namespace {

constexpr int kMclMaxK = 64;                    // SELHIP_MCL_MAX_ENTRIES
constexpr int kMclStartCap = 4096;              // longest row, its self loop included, that mcl_start_kernel orders in LDS
constexpr int kMclStartBlock = 256;
static_assert(kMclMaxK == SELHIP_MCL_MAX_ENTRIES && kMclMaxK == kWave, "a key keeps 6 bits each for the slot and the entry; wave 0 finishes a column");

template <int KCLASS> struct MclGeom;
template <> struct MclGeom<0> { static constexpr int kK = 8, kThreads = kBlock, kCap = kWave; };
template <> struct MclGeom<1> { static constexpr int kK = 32, kThreads = 256, kCap = 1024; };
template <> struct MclGeom<2> { static constexpr int kK = 64, kThreads = 512, kCap = 4096; };

struct MclEll { int* row; double* val; int* cnt; };         // [n * K], [n * K], [n]

// the LDS of a workgroup that orders up to `cap` candidates: 12 bytes each, and the column's own arrays
struct MclLds {
    u64* sa; u64* smax; double* w; double* wval; uint32_t* sb; int* ks; uint32_t* soff; int* wrow;
    __device__ __forceinline__ MclLds(unsigned char* base, int cap) {
        sa = reinterpret_cast<u64*>(base);                  // [cap]  sort key, then the bits of the inflated value
        smax = sa + cap;                                    // the column's largest inflated value, as bits
        w = reinterpret_cast<double*>(smax + 1);            // [64]   the column's own values w_s
        wval = w + kMclMaxK;                                // [64]   the survivors by ascending row
        sb = reinterpret_cast<uint32_t*>(wval + kMclMaxK);  // [cap]  the row behind sa
        ks = reinterpret_cast<int*>(sb + cap);              // [64]   the column's own rows k_s: the source columns
        soff = reinterpret_cast<uint32_t*>(ks + kMclMaxK);  // [65]   where source s starts among the products
        wrow = reinterpret_cast<int*>(soff + kMclMaxK + 1); // [64]
    }
};
constexpr size_t mcl_lds_bytes(int cap) { return (size_t)cap * 12 + 8 + 2 * kMclMaxK * 8 + kMclMaxK * 4 + (kMclMaxK + 1) * 4 + kMclMaxK * 4; }
static_assert(mcl_lds_bytes(MclGeom<1>::kCap) == 14092 && mcl_lds_bytes(MclGeom<2>::kCap) == 50956 && mcl_lds_bytes(kMclStartCap) <= 64 * 1024, "LDS per class");

__device__ __forceinline__ u64 mcl_bits(double v) { return (u64)__double_as_longlong(v); }
__device__ __forceinline__ double mcl_double(u64 b) { return __longlong_as_double((long long)b); }
__device__ __forceinline__ double mcl_inflate(double x, double r) { return r == 2.0 ? __dmul_rn(x, x) : pow(x, r); }

// ORDER 0: a ascending (the product keys: all different).  ORDER 1: "best": a descending, equal a by ascending b
template <int ORDER>
__device__ __forceinline__ bool mcl_before(u64 a0, uint32_t b0, u64 a1, uint32_t b1) {
    if constexpr (ORDER == 0) return a0 < a1;
    else return a0 > a1 || (a0 == a1 && b0 < b1);
}

// (sa, sb)[0, L) in LDS into ORDER by the whole workgroup: the network of kernel_adjacency.cuh, positions at or past L never move.
// Complete before the call (a barrier stands in front of it), settled behind it
template <int ORDER, int THREADS>
__device__ __forceinline__ void mcl_lds_sort(u64* sa, uint32_t* sb, uint32_t L) {
    uint32_t n = 1;
    while (n < L) n <<= 1;
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool first = j == (k >> 1);
            for (uint32_t q = threadIdx.x; q < (n >> 1); q += THREADS) {
                const uint32_t lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const uint32_t hi = first ? lo ^ (k - 1) : lo | j;
                if (hi < L) {
                    const u64 a0 = sa[lo], a1 = sa[hi];
                    const uint32_t b0 = sb[lo], b1 = sb[hi];
                    if (mcl_before<ORDER>(a1, b1, a0, b0)) { sa[lo] = a1; sb[lo] = b1; sa[hi] = a0; sb[hi] = b0; }
                }
            }
            __syncthreads();
        }
    }
}

// one entry per lane, (a, b) with b's low 32 bits the row under ORDER 1 and any payload under ORDER 0, into ORDER across the wave
template <int ORDER>
__device__ __forceinline__ void mcl_wave_sort(u64& a, u64& b, int lane) {
    const auto step = [&](int mask, int bit) {
        const u64 oa = (u64)__shfl_xor((long long)a, mask, kWave), ob = (u64)__shfl_xor((long long)b, mask, kWave);
        const bool lower = (lane & bit) == 0;
        if (lower ? mcl_before<ORDER>(oa, (uint32_t)ob, a, (uint32_t)b) : mcl_before<ORDER>(a, (uint32_t)b, oa, (uint32_t)ob)) { a = oa; b = ob; }
    };
#pragma unroll
    for (int k = 2; k <= kWave; k <<= 1) {
        step(k - 1, k >> 1);
#pragma unroll
        for (int j = k >> 2; j > 0; j >>= 1) step(j, j);
    }
}

// bad[0]: entries whose value is not finite or < 0, whose column lies outside [0, n) or is not above its predecessor's in the row;
// bad[1]: rows whose offsets do not ascend inside [0, nnz] from 0.  One lane per entry for the values and the range; one wave per row
// for the offsets and, where they hold, the order of the row's columns.  Reads only col / val [0, nnz) and row_ptr [0, n]
__global__ __launch_bounds__(kBlock)
void mcl_check_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const double* __restrict__ val, long long n, long long nnz,
                      ClusterBad* __restrict__ bad) {
    const long long stride = (long long)gridDim.x * kBlock, t0 = (long long)blockIdx.x * kBlock + threadIdx.x;
    for (long long e = t0; e < nnz; e += stride) {
        const double v = val[e];
        if (!(v >= 0.0) || v == INFINITY || (u64)(uint32_t)col[e] >= (u64)n) { atomicAdd(&bad[0].count, 1ull); atomicMin(&bad[0].index, (u64)e); }
    }
    const int lane = threadIdx.x & (kWave - 1);
    for (long long r = t0 / kWave; r < n; r += stride / kWave) {
        const int64_t a = row_ptr[r], b = row_ptr[r + 1];
        if (a < 0 || b < a || b > nnz || (r == 0 && a != 0)) {
            if (lane == 0) { atomicAdd(&bad[1].count, 1ull); atomicMin(&bad[1].index, (u64)r); }
            continue;                                       // (the same for the whole wave)
        }
        for (int64_t e = a + 1 + lane; e < b; e += kWave)
            if (col[e] <= col[e - 1]) { atomicAdd(&bad[0].count, 1ull); atomicMin(&bad[0].index, (u64)e); }
    }
}

// (sa, sb)[0, lim), lim <= K: a column's candidates best first, the slots without one (sa == 0) behind the others.  Ranks the kept ones by
// row, adds them in ascending row order, divides, writes column j of `out` and returns the column's chaos to thread 0.  Called by every
// thread behind a barrier; the work is wave 0's
__device__ __forceinline__ double mcl_finish(const MclLds& l, uint32_t lim, int K, const MclEll& out, int j) {
    const int tid = threadIdx.x;
    uint32_t kk = 0;
    if (tid < kWave) {
        const bool valid = (uint32_t)tid < lim && l.sa[tid] != 0;
        kk = (uint32_t)__popcll(__ballot(valid));
        if (valid) {
            const uint32_t row = l.sb[tid];
            uint32_t rank = 0;
            for (uint32_t e = 0; e < kk; ++e) rank += l.sb[e] < row ? 1u : 0u;
            l.wrow[rank] = (int)row; l.wval[rank] = mcl_double(l.sa[tid]);
        }
    }
    __syncthreads();
    double y = 0.0;
    if (tid < kWave && kk > 0) {
        double s = l.wval[0];
        for (uint32_t e = 1; e < kk; ++e) s = __dadd_rn(s, l.wval[e]);
        if ((uint32_t)tid < kk) y = __ddiv_rn(l.wval[tid], s);
    }
    __syncthreads();
    if ((uint32_t)tid < kk) {                               // (kk is 0 outside wave 0)
        l.wval[tid] = y;
        out.row[(size_t)j * K + tid] = l.wrow[tid]; out.val[(size_t)j * K + tid] = y;
    }
    __syncthreads();
    double chaos = 0.0;
    if (tid == 0) {
        out.cnt[j] = (int)kk;
        if (kk > 0) {
            double mx = l.wval[0], sq = __dmul_rn(mx, mx);
            for (uint32_t e = 1; e < kk; ++e) { const double v = l.wval[e]; mx = v > mx ? v : mx; sq = __dadd_rn(sq, __dmul_rn(v, v)); }
            chaos = __dsub_rn(mx, sq);
        }
    }
    return chaos;
}

// one workgroup per CSR row.  Entries of value 0 and the diagonal's are no candidates; the self loop carries the row's largest value
__global__ __launch_bounds__(kMclStartBlock)
void mcl_start_kernel(const int64_t* __restrict__ row_ptr, const int32_t* __restrict__ col, const double* __restrict__ val, int n, int K, MclEll out) {
    extern __shared__ __attribute__((aligned(16))) unsigned char mcl_smem[];
    const MclLds l(mcl_smem, kMclStartCap);
    const int tid = threadIdx.x;
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        const int64_t s0 = row_ptr[j], L = row_ptr[j + 1] - s0;
        if (tid == 0) *l.smax = 0;
        __syncthreads();
        u64 mine = 0;
        for (int64_t t = tid; t < L; t += kMclStartBlock) {
            const double v = val[s0 + t];
            if (col[s0 + t] != j && v > 0.0 && mcl_bits(v) > mine) mine = mcl_bits(v);
        }
        if (mine) atomicMax(l.smax, mine);
        __syncthreads();
        const u64 top = *l.smax;
        const u64 self = top ? top : mcl_bits(1.0);
        uint32_t lim;
        if (L + 1 <= (int64_t)kMclStartCap) {
            for (int64_t t = tid; t < L; t += kMclStartBlock) {
                const int c = col[s0 + t];
                const double v = val[s0 + t];
                l.sa[t] = c != j && v > 0.0 ? mcl_bits(v) : 0ull; l.sb[t] = (uint32_t)c;
            }
            if (tid == 0) { l.sa[L] = self; l.sb[L] = (uint32_t)j; }
            __syncthreads();
            mcl_lds_sort<1, kMclStartBlock>(l.sa, l.sb, (uint32_t)(L + 1));
            lim = (uint32_t)(L + 1 < (int64_t)K ? L + 1 : (int64_t)K);
        } else {
            // the long route: round q finds the best candidate behind winner q - 1 in the order -- the largest value among them, then the
            // smallest row among its holders -- in two passes over the row.  soff[0] is the round's row, smax its value: the rounds
            // rewrite smax, so every thread has read the row's largest value (`top`) before the first of them begins
            u64 pa = ~0ull;
            uint32_t pb = 0;
            if (tid < K) { l.sa[tid] = 0; l.sb[tid] = 0xFFFFFFFFu; }
            __syncthreads();
            for (int q = 0; q < K; ++q) {
                if (tid == 0) { *l.smax = 0; l.soff[0] = 0xFFFFFFFFu; }
                __syncthreads();
                u64 la = 0;
                uint32_t lb = 0xFFFFFFFFu;
                for (int64_t t = tid; t <= L; t += kMclStartBlock) {        // (t == L: the self loop)
                    const uint32_t b = t < L ? (uint32_t)col[s0 + t] : (uint32_t)j;
                    const double v = t < L ? val[s0 + t] : 0.0;
                    const u64 a = t == L ? self : (b != (uint32_t)j && v > 0.0 ? mcl_bits(v) : 0ull);
                    if (a != 0 && mcl_before<1>(pa, pb, a, b) && mcl_before<1>(a, b, la, lb)) { la = a; lb = b; }
                }
                if (la) atomicMax(l.smax, la);
                __syncthreads();
                const u64 ga = *l.smax;
                if (ga == 0) break;                                         // (the same for every thread)
                if (la == ga) atomicMin(&l.soff[0], lb);
                __syncthreads();
                const uint32_t gb = l.soff[0];
                if (tid == 0) { l.sa[q] = ga; l.sb[q] = gb; }
                pa = ga; pb = gb;
                __syncthreads();
            }
            __syncthreads();
            lim = (uint32_t)K;
        }
        (void)mcl_finish(l, lim, K, out, j);
        __syncthreads();
    }
}

// the iteration of the columns a wave owns, K <= 8: everything in registers
__device__ __forceinline__ void mcl_step_wave(const MclEll& in, const MclEll& out, int n, int K, double r, double prune, u64* __restrict__ chaos_now) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    for (u64 j = wave; j < (u64)n; j += waves) {
        int c = in.cnt[j];
        c = c < 0 ? 0 : c > MclGeom<0>::kK ? MclGeom<0>::kK : c;
        int ks = 0;
        double w = 0.0;
        uint32_t inc = 0;
        if (lane < c) { ks = in.row[j * K + lane]; w = in.val[j * K + lane]; inc = (uint32_t)in.cnt[ks]; inc = inc > (uint32_t)K ? (uint32_t)K : inc; }
#pragma unroll
        for (int d = 1; d < MclGeom<0>::kK; d <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, d, kWave); if (lane >= d) inc += o; }
        // lane p holds product p: entry p - start of the source s whose range [start, end) holds p
        int s = 0;
        uint32_t start = 0, P = 0;
#pragma unroll
        for (int e = 0; e < MclGeom<0>::kK; ++e) {
            const uint32_t end = (uint32_t)__shfl((int)inc, e, kWave);
            if (e < c && end <= (uint32_t)lane) { s = e + 1; start = end; }
            if (e == MclGeom<0>::kK - 1) P = end;
        }
        const bool have = (uint32_t)lane < P;               // (then s < c)
        const int ks_s = __shfl(ks, s, kWave);
        const double w_s = __shfl(w, s, kWave);
        u64 a = ~0ull, b = 0;
        if (have) {
            const uint32_t t = (uint32_t)lane - start;
            const size_t at = (size_t)ks_s * K + t;
            a = ((u64)(uint32_t)in.row[at] << 12) | ((u64)s << 6) | (u64)t;
            b = mcl_bits(__dmul_rn(in.val[at], w_s));
        }
        mcl_wave_sort<0>(a, b, lane);
        // the head of a run of equal rows adds its run, at most c products, in the order they lie in: ascending s
        const u64 row = a >> 12;
        const u64 prev = (u64)__shfl_up((long long)row, 1, kWave);
        const bool head = have && (lane == 0 || prev != row);
        double acc = mcl_double(b);
#pragma unroll
        for (int e = 1; e < MclGeom<0>::kK; ++e) {
            const int src = lane + e < kWave ? lane + e : lane;
            const u64 orow = (u64)__shfl((long long)row, src, kWave);
            const double oprod = __shfl(mcl_double(b), src, kWave);
            if (lane + e < kWave && (uint32_t)(lane + e) < P && orow == row) acc = __dadd_rn(acc, oprod);
        }
        u64 xa = head ? mcl_bits(mcl_inflate(acc, r)) : 0ull;
        u64 top = xa;
#pragma unroll
        for (int m = 1; m < kWave; m <<= 1) { const u64 o = (u64)__shfl_xor((long long)top, m, kWave); top = o > top ? o : top; }
        if (mcl_double(xa) < __dmul_rn(prune, mcl_double(top))) xa = 0;
        u64 xb = xa ? row : 0xFFFFFFFFull;
        mcl_wave_sort<1>(xa, xb, lane);
        const bool valid = lane < K && xa != 0;
        const int kk = (int)__popcll(__ballot(valid));
        int rank = 0;
#pragma unroll
        for (int e = 0; e < MclGeom<0>::kK; ++e) {
            const uint32_t rb = (uint32_t)__shfl((int)(uint32_t)xb, e, kWave);
            if (e < kk && rb < (uint32_t)xb) ++rank;
        }
        // the sum in ascending row order: rank by rank, every lane adds the same numbers
        const double x = mcl_double(xa);
        double sum = 0.0;
        for (int q = 0; q < kk; ++q) {
            const int src = __ffsll((long long)__ballot(valid && rank == q)) - 1;
            const double xq = __shfl(x, src, kWave);
            sum = q == 0 ? xq : __dadd_rn(sum, xq);
        }
        const double y = valid ? __ddiv_rn(x, sum) : 0.0;
        double mx = 0.0, sq = 0.0;
        for (int q = 0; q < kk; ++q) {
            const int src = __ffsll((long long)__ballot(valid && rank == q)) - 1;
            const double yq = __shfl(y, src, kWave);
            mx = q == 0 || yq > mx ? yq : mx;
            sq = q == 0 ? __dmul_rn(yq, yq) : __dadd_rn(sq, __dmul_rn(yq, yq));
        }
        if (valid) { out.row[j * K + rank] = (int)(uint32_t)xb; out.val[j * K + rank] = y; }
        if (lane == 0) { out.cnt[j] = kk; atomicMax(chaos_now, graph_image(__dsub_rn(mx, sq))); }
    }
}

// the iteration of the columns a workgroup owns, K <= 32 (KCLASS 1) or K <= 64 (KCLASS 2): products and candidates in LDS
template <int KCLASS>
__device__ __forceinline__ void mcl_step_block(const MclEll& in, const MclEll& out, int n, int K, double r, double prune, u64* __restrict__ chaos_now) {
    constexpr int T = MclGeom<KCLASS>::kThreads, CAP = MclGeom<KCLASS>::kCap, PER = CAP / T;
    extern __shared__ __attribute__((aligned(16))) unsigned char mcl_smem[];
    const MclLds l(mcl_smem, CAP);
    const int tid = threadIdx.x;
    for (int j = blockIdx.x; j < n; j += gridDim.x) {
        int c = in.cnt[j];
        c = c < 0 ? 0 : c > K ? K : c;
        if (tid < c) {
            const int ks = in.row[(size_t)j * K + tid];
            const int sc = in.cnt[ks];
            l.ks[tid] = ks; l.w[tid] = in.val[(size_t)j * K + tid]; l.soff[tid + 1] = (uint32_t)(sc < 0 ? 0 : sc > K ? K : sc);
        }
        if (tid == 0) { l.soff[0] = 0; *l.smax = 0; }
        __syncthreads();
        if (tid == 0) for (int s = 0; s < c; ++s) l.soff[s + 1] += l.soff[s];
        __syncthreads();
        const uint32_t P = l.soff[c] < (uint32_t)CAP ? l.soff[c] : (uint32_t)CAP;   // (c <= K entries of <= K each: never clipped)
        for (uint32_t p = tid; p < P; p += T) {
            int lo = 0, hi = c - 1;                         // the source s with soff[s] <= p < soff[s + 1]
            while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (l.soff[mid] <= p) lo = mid; else hi = mid - 1; }
            const uint32_t t = p - l.soff[lo];
            l.sa[p] = ((u64)(uint32_t)in.row[(size_t)l.ks[lo] * K + t] << 12) | ((u64)lo << 6) | (u64)t;
            l.sb[p] = 0;
        }
        __syncthreads();
        mcl_lds_sort<0, T>(l.sa, l.sb, P);
        // slot q = tid + u T: the head of a run of equal rows adds its run -- at most c products, ascending s -- and inflates the sum
        u64 xa[PER];
        uint32_t xrow[PER];
        u64 best = 0;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const uint32_t q = (uint32_t)tid + (uint32_t)u * T;
            xa[u] = 0; xrow[u] = 0xFFFFFFFFu;
            if (q < P) {
                const u64 row = l.sa[q] >> 12;
                if (q == 0 || (l.sa[q - 1] >> 12) != row) {
                    double acc = 0.0;
                    for (uint32_t e = q; e < P; ++e) {
                        const u64 ke = l.sa[e];
                        if ((ke >> 12) != row) break;
                        const int s = (int)((ke >> 6) & 63u);
                        const double prod = __dmul_rn(in.val[(size_t)l.ks[s] * K + (ke & 63u)], l.w[s]);
                        acc = e == q ? prod : __dadd_rn(acc, prod);
                    }
                    xa[u] = mcl_bits(mcl_inflate(acc, r)); xrow[u] = (uint32_t)row;
                    best = xa[u] > best ? xa[u] : best;
                }
            }
        }
        if (best) atomicMax(l.smax, best);
        __syncthreads();                                    // every key has been read, the column's largest value is in
        const double cut = __dmul_rn(prune, mcl_double(*l.smax));
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const uint32_t q = (uint32_t)tid + (uint32_t)u * T;
            if (q < P) {
                const bool keep = xa[u] != 0 && !(mcl_double(xa[u]) < cut);
                l.sa[q] = keep ? xa[u] : 0ull; l.sb[q] = keep ? xrow[u] : 0xFFFFFFFFu;
            }
        }
        __syncthreads();
        mcl_lds_sort<1, T>(l.sa, l.sb, P);
        const double chaos = mcl_finish(l, P < (uint32_t)K ? P : (uint32_t)K, K, out, j);
        if (tid == 0) atomicMax(chaos_now, graph_image(chaos));
        __syncthreads();
    }
}

// chaos_now: the maximum of this iteration's column chaos images, 0 on entry; chaos_next: the slot of the next iteration, cleared here
// (the host has read it: it waits for every iteration's chaos before it enqueues the next)
template <int KCLASS>
__global__ __launch_bounds__(MclGeom<KCLASS>::kThreads)
void mcl_step_kernel(MclEll in, MclEll out, int n, int K, double r, double prune, u64* __restrict__ chaos_now, u64* __restrict__ chaos_next) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *chaos_next = 0;
    if constexpr (KCLASS == 0) mcl_step_wave(in, out, n, K, r, prune, chaos_now);
    else mcl_step_block<KCLASS>(in, out, n, K, r, prune, chaos_now);
}

// the final matrix as an edge list for the union-find of kernel_graph.cuh: slot e = (column e / K, entry e % K) is the edge {row, column}
struct MclEdgeList {
    const int* row; const int* cnt; int K;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v, double* value) const {
        const u64 j = e / (u64)K;
        if ((int)(e - j * (u64)K) >= cnt[j]) return false;
        *u = row[e]; *v = (int)j; *value = 1.0;
        return true;
    }
};

}  // namespace

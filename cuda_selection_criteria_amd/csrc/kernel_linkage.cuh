// kernel_linkage.cuh -- agglomerative hierarchy (single, complete, average = UPGMA, weighted = WPGMA linkage) of a dense f64 distance
// matrix in rounds of reciprocal nearest neighbours (selhip_linkage, selhip_ctx_linkage; include/selection_hip.h section 2k, host side
// in host_linkage.hpp).  Part of libselhip.so; included by selection_kernels.hip only, behind kernel_forest.cuh (ClusterBad, ForestEdge).
//
// STATE.  D[n][ld] f64, bit-symmetric behind lk_mirror_kernel; active[s], size[s]; a cluster lives in the slot of its smallest member;
// nn[s] / nd[s] the cached nearest neighbour of row s and its distance.  The DIRTY rows of a round are a list (list[0 .. words[0])),
// written by the kernel that makes them dirty, so a round scans only them and no flag array has to be cleared.
//
// A ROUND (the host reads two words per round, host_linkage.hpp):
//   lk_scan_kernel    one workgroup per dirty row: argmin over the active columns b != r under (value, slot) -- f64 `<`, equal values
//                     (-0.0 and +0.0 are equal) to the smaller slot.  Inactive columns are masked from active[]: +inf is data
//   lk_pair_kernel    ONE workgroup: paired[s] for every slot (s and t = nn[s] active, nn[t] == s, nd[min(s, t)] <= max_height), the
//                     pairs' smaller slots compacted in ascending order, and with them the merge records and new sizes behind the
//                     F records of the rounds before
//   lk_update_kernel  one work item per (pair, column k): the Lance-Williams value of the merged row, read along rows a and b, stored
//                     at [a][k] and mirrored to [k][a].  In place: a cell one item writes is read by no other item of the launch
//                     (rows of b slots and of unpaired slots are never written as rows; [a][k] is read by its own item alone)
//   lk_book_kernel    one lane per slot: size[a] += size[b], b inactive, and the next round's dirty list: every a, and every active
//                     row whose cached neighbour is in a pair of this round
// lk_all_kernel lists every active row (round 1, and a rescan round: no pair although not every row was scanned).
//
// ARITHMETIC.  lk_lw rounds every product, sum and quotient on its own (no contraction), sizes as doubles; it is the one definition
// of the update, called once for a survivor in no pair and three times for a survivor that is itself a pair.
//
// ORDER.  The dirty list's order is that of an atomic add and differs from run to run; a row's scan depends on its row alone.  The
// pairs are compacted by one workgroup in ascending slot order, so every output is a pure function of the input.
// No loop waits for another lane, wave or block; no cooperative launch; visibility between the launches is the kernel boundary's.
#pragma once

namespace {

constexpr int kLkScanCols = 2 * kBlock;          // columns one sweep of a row-scan workgroup covers on the 16-byte path
constexpr int kLkPairBlock = 1024;               // the one workgroup of lk_pair_kernel
constexpr int kLkTile = 32;                      // lk_mirror_kernel: a 32 x 32 tile per workgroup of 32 x 8 threads
constexpr int kLkWords = 4;                      // [0] rows on the dirty list, [1] pairs of the round, [2] records emitted so far

// every slot active, size 1, no cached neighbour; the words cleared
__global__ void __launch_bounds__(kBlock)
lk_init_kernel(int n, uint8_t* __restrict__ active, int* __restrict__ size, int* __restrict__ nn, double* __restrict__ nd, uint32_t* __restrict__ words,
               ClusterBad* __restrict__ bad) {
    const int stride = (int)gridDim.x * kBlock;
    for (int s = (int)blockIdx.x * kBlock + (int)threadIdx.x; s < n; s += stride) { active[s] = 1; size[s] = 1; nn[s] = -1; nd[s] = 0.0; }
    if (blockIdx.x == 0 && threadIdx.x < kLkWords) words[threadIdx.x] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { bad->count = 0; bad->index = ~0ull; }
}

// the strict upper triangle mirrored into the lower one through an LDS tile (both sides coalesced); a NaN or -inf cell of the upper
// triangle is tallied in *bad with the smallest a * n + b.  Tiles below the diagonal return at once
__global__ void __launch_bounds__(kBlock)
lk_mirror_kernel(double* __restrict__ D, long long ld, int n, ClusterBad* __restrict__ bad) {
    const int ti = (int)blockIdx.y, tj = (int)blockIdx.x;
    if (ti > tj) return;
    __shared__ double tile[kLkTile][kLkTile + 1];
    const int tx = (int)threadIdx.x % kLkTile, ty = (int)threadIdx.x / kLkTile;
    u64 n_bad = 0, first = ~0ull;
    for (int r = ty; r < kLkTile; r += kBlock / kLkTile) {
        const int a = ti * kLkTile + r, b = tj * kLkTile + tx;
        double v = 0.0;
        if (a < n && b < n && a < b) {
            v = D[(long long)a * ld + b];
            if (!(v > -INFINITY)) { ++n_bad; const u64 at = (u64)a * (u64)n + (u64)b; first = at < first ? at : first; }
        }
        tile[r][tx] = v;
    }
    __syncthreads();
    for (int r = ty; r < kLkTile; r += kBlock / kLkTile) {
        const int b = tj * kLkTile + r, a = ti * kLkTile + tx;
        if (a < n && b < n && a < b) D[(long long)b * ld + a] = tile[tx][r];
    }
    if (n_bad) { atomicAdd(&bad->count, n_bad); atomicMin(&bad->index, first); }
}

// the distance of a similarity, in place over the whole square: 1 - v, and 1.0 for a NaN (two empty sketches under the HLL measures)
__global__ void __launch_bounds__(kBlock)
lk_distance_kernel(double* __restrict__ D, long long cells) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long e = (long long)blockIdx.x * kBlock + threadIdx.x; e < cells; e += stride) {
        const double v = D[e];
        D[e] = v == v ? 1.0 - v : 1.0;
    }
}

// list[] = the active slots (any order), words[0] their number.  words[0] is 0 on entry
__global__ void __launch_bounds__(kBlock)
lk_all_kernel(int n, const uint8_t* __restrict__ active, int* __restrict__ list, uint32_t* __restrict__ words) {
    const int lane = (int)__lane_id();
    const int stride = (int)gridDim.x * kBlock;
    for (int base = (int)blockIdx.x * kBlock; base < n; base += stride) {          // block-uniform bound: the waves stay whole
        const int s = base + (int)threadIdx.x;
        const bool on = s < n && active[s];
        const u64 m = __ballot(on);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(words, (uint32_t)__popcll(m));
            first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
            if (on) list[first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = s;
        }
    }
}

// (v2, c2) replaces (v1, c1): c < 0 is "none yet"
__device__ __forceinline__ bool lk_better(double v1, int c1, double v2, int c2) { return c2 >= 0 && (c1 < 0 || v2 < v1 || (v2 == v1 && c2 < c1)); }

// kWide: ld even and the base 16-byte aligned, so every row is: two columns per load.  A lane visits its columns in ascending order,
// so inside a lane `<` alone keeps the smaller slot among equal values
template <bool kWide>
__global__ void __launch_bounds__(kBlock)
lk_scan_kernel(const double* __restrict__ D, long long ld, int n, const uint8_t* __restrict__ active, const int* __restrict__ list,
               int* __restrict__ nn, double* __restrict__ nd) {
    const int r = list[blockIdx.x];
    const double* __restrict__ row = D + (long long)r * ld;
    double bv = 0.0;
    int bc = -1;
    if (kWide) {
#pragma unroll 4
        for (int c = 2 * (int)threadIdx.x; c < n; c += kLkScanCols) {
            if (c + 1 < n) {
                const double2 v = *reinterpret_cast<const double2*>(row + c);
                const uint32_t on = *reinterpret_cast<const uint16_t*>(active + c);        // (c is even and active[] 16-byte aligned)
                if ((on & 0xFFu) && c != r && (bc < 0 || v.x < bv)) { bv = v.x; bc = c; }
                if ((on >> 8) && c + 1 != r && (bc < 0 || v.y < bv)) { bv = v.y; bc = c + 1; }
            } else {
                const double v = row[c];
                if (active[c] && c != r && (bc < 0 || v < bv)) { bv = v; bc = c; }
            }
        }
    } else {
#pragma unroll 4
        for (int c = (int)threadIdx.x; c < n; c += kBlock) {
            const double v = row[c];
            if (active[c] && c != r && (bc < 0 || v < bv)) { bv = v; bc = c; }
        }
    }
    for (int s = kWave / 2; s; s >>= 1) {
        const double ov = __shfl_xor(bv, s);
        const int oc = __shfl_xor(bc, s);
        if (lk_better(bv, bc, ov, oc)) { bv = ov; bc = oc; }
    }
    __shared__ double wv[kWavesPerBlock];
    __shared__ int wc[kWavesPerBlock];
    if (__lane_id() == 0) { wv[threadIdx.x / kWave] = bv; wc[threadIdx.x / kWave] = bc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kWavesPerBlock; ++w)
            if (lk_better(bv, bc, wv[w], wc[w])) { bv = wv[w]; bc = wc[w]; }
        nn[r] = bc;
        nd[r] = bc < 0 ? 0.0 : bv;
    }
}

// launched as one workgroup.  cap: the records d_merges holds (n - 1); a store never depends on F staying below it
__global__ void __launch_bounds__(kLkPairBlock)
lk_pair_kernel(int n, const uint8_t* __restrict__ active, const int* __restrict__ nn, const double* __restrict__ nd, const int* __restrict__ size,
               double max_height, uint8_t* __restrict__ paired, selhip_int2_t* __restrict__ pairs, ForestEdge* __restrict__ merges,
               int* __restrict__ msize, uint32_t cap, uint32_t* __restrict__ words) {
    __shared__ uint32_t wsum[kLkPairBlock / kWave];
    const int lane = (int)__lane_id(), wave = (int)threadIdx.x / kWave;
    const uint32_t f = words[2];
    uint32_t base = 0;
    for (int s0 = 0; s0 < n; s0 += kLkPairBlock) {
        const int s = s0 + (int)threadIdx.x;
        bool in_pair = false, first = false;
        int t = -1;
        if (s < n && active[s]) {
            t = nn[s];
            if (t >= 0 && active[t] && nn[t] == s) {
                in_pair = nd[s < t ? s : t] <= max_height;
                first = in_pair && s < t;
            }
        }
        if (s < n) paired[s] = in_pair ? 1 : 0;
        const u64 m = __ballot(first);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < kLkPairBlock / kWave; ++w) { const uint32_t x = wsum[w]; total += x; if (w < wave) before += x; }
        __syncthreads();
        if (first) {
            const uint32_t idx = base + before + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            pairs[idx] = selhip_int2_t{s, t};
            if (f + idx < cap) {
                const u64 bits = (u64)__double_as_longlong(nd[s]);
                reinterpret_cast<uint4*>(merges)[f + idx] = make_uint4((uint32_t)s, (uint32_t)t, (uint32_t)bits, (uint32_t)(bits >> 32));
                msize[f + idx] = size[s] + size[t];
            }
        }
        base += total;
    }
    if (threadIdx.x == 0) { words[0] = 0; words[1] = base; words[2] = f + base; }
}

// the Lance-Williams value of d(i u j, k) from x = d(i, k), y = d(j, k) and the two sizes, every operation rounded on its own
__device__ __forceinline__ double lk_lw(int method, double x, double y, double sa, double sb) {
#pragma clang fp contract(off)
    switch (method) {
        case SELHIP_LINKAGE_SINGLE:   return y < x ? y : x;
        case SELHIP_LINKAGE_COMPLETE: return y > x ? y : x;
        case SELHIP_LINKAGE_AVERAGE: {
            const double px = sa * x, py = sb * y, s = sa + sb;
            const double num = px + py;
            return num / s;
        }
        default: {
            const double hx = 0.5 * x, hy = 0.5 * y;
            return hx + hy;
        }
    }
}

// grid: (column blocks, pair blocks); a workgroup takes the pairs blockIdx.y, + gridDim.y, ...
__global__ void __launch_bounds__(kBlock)
lk_update_kernel(double* D, long long ld, int n, int method, const uint8_t* __restrict__ active, const uint8_t* __restrict__ paired,
                 const int* __restrict__ nn, const int* __restrict__ size, const selhip_int2_t* __restrict__ pairs, uint32_t n_pairs) {
    const int k = (int)blockIdx.x * kBlock + (int)threadIdx.x;
    if (k >= n || !active[k]) return;
    for (uint32_t p = blockIdx.y; p < n_pairs; p += gridDim.y) {
        const int a = pairs[p].x, b = pairs[p].y;
        if (k == a || k == b) continue;
        const double sa = (double)size[a], sb = (double)size[b];
        double* const row_a = D + (long long)a * ld;
        const double* const row_b = D + (long long)b * ld;
        double v;
        if (!paired[k]) {
            v = lk_lw(method, row_a[k], row_b[k], sa, sb);
        } else {
            const int d = nn[k];
            if (k > d || k < a) continue;                       // the pair's larger slot dies; the pair with the smaller a computes the cell
            const double sc = (double)size[k], sd = (double)size[d];
            v = lk_lw(method, lk_lw(method, row_a[k], row_a[d], sc, sd), lk_lw(method, row_b[k], row_b[d], sc, sd), sa, sb);
        }
        row_a[k] = v;
        D[(long long)k * ld + a] = v;
    }
}

// words[0] is 0 on entry (lk_pair_kernel)
__global__ void __launch_bounds__(kBlock)
lk_book_kernel(int n, uint8_t* __restrict__ active, const uint8_t* __restrict__ paired, const int* __restrict__ nn, int* __restrict__ size,
               int* __restrict__ list, uint32_t* __restrict__ words) {
    const int lane = (int)__lane_id();
    const int stride = (int)gridDim.x * kBlock;
    for (int base = (int)blockIdx.x * kBlock; base < n; base += stride) {
        const int s = base + (int)threadIdx.x;
        bool dirty = false;
        if (s < n && active[s]) {
            const int t = nn[s];
            if (paired[s]) {
                if (s < t) { size[s] += size[t]; dirty = true; }   // (size[t] is a dying slot's: nothing writes it)
                else active[s] = 0;
            } else {
                dirty = t >= 0 && paired[t];
            }
        }
        const u64 m = __ballot(dirty);
        if (m) {
            const int leader = __ffsll((long long)m) - 1;
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(words, (uint32_t)__popcll(m));
            first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
            if (dirty) list[first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = s;
        }
    }
}

}  // namespace

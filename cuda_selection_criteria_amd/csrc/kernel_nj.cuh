// kernel_nj.cuh -- the neighbour-joining tree of a dense f64 distance matrix (selhip_neighbor_joining, selhip_ctx_neighbor_joining;
// include/selection_hip.h section 2l holds THE DEFINITION, host side in host_nj.hpp).  Part of libselhip.so; included by
// selection_kernels.hip only, behind kernel_linkage.cuh (ClusterBad, kLkTile, lk_distance_kernel).
//
// STATE.  D[n][ld] f64, bit-symmetric behind nj_mirror_kernel; active[s]; R[s] the row sums; list[0 .. r) the active slots in
// ASCENDING order (two buffers, one read and one written per join, so the repair is a plain shift and a workgroup's rows are
// neighbours in the triangle); best_q / best_b per list position; NjPick = what the pick publishes for the update.
//
// A JOIN over r active slots is three launches, back to back, with no host read in between (the host knows r = n - s):
//   nj_scan_kernel    a workgroup takes kNjRows consecutive rows of the list and sweeps the columns behind the first of them ONCE:
//                     R[c] and active[c] are read once per sweep step (from L2: the two vectors are n long and every workgroup
//                     reads them) and stay in registers for the kNjRows matrix loads that go with them (16-byte loads on the kWide
//                     path), so the matrix is the only HBM stream and the vectors cost 1 / kNjRows of its requests.  q is formed
//                     per cell, a lane keeps one best (q, b) per row, a wave butterfly and one LDS step reduce them
//   nj_pick_kernel    ONE workgroup of kNjSum lanes: the best row under (q, a, b), the record, then -- reading rows a and b as they
//                     still are -- the fresh sum of the new row in the contract's shape, stored as R[a]
//   nj_update_kernel  one lane per column k (cluster_vertex_grid): v, both mirrored cells, R[k]; b retired; the list shifted
// The last join (r == 2) has no update.
//
// ORDER.  Every reduction is under a total order -- (q, b) in a row, (q, a, b) across rows -- and the row sum has one fixed shape
// (nj_row_sum below), so every output is a pure function of the upper triangle.  No floating-point atomics, no loop that waits for
// another lane, wave or block, no cooperative launch; visibility between the launches is the kernel boundary's.
#pragma once

namespace {

constexpr int kNjRows = 4;                       // list rows one scan workgroup takes
constexpr int kNjScanCols = 2 * kBlock;          // columns one sweep step of a scan workgroup covers on the 16-byte path
constexpr int kNjSum = 1024;                     // lanes of THE row sum: nj_rowsum_kernel's and nj_pick_kernel's workgroup

struct NjPick { int a, b; double d; };

// every slot active, the list 0 .. n - 1, the refusal tally cleared
__global__ void __launch_bounds__(kBlock)
nj_init_kernel(int n, uint8_t* __restrict__ active, int* __restrict__ list, ClusterBad* __restrict__ bad) {
    const int stride = (int)gridDim.x * kBlock;
    for (int s = (int)blockIdx.x * kBlock + (int)threadIdx.x; s < n; s += stride) { active[s] = 1; list[s] = s; }
    if (blockIdx.x == 0 && threadIdx.x == 0) { bad->count = 0; bad->index = ~0ull; }
}

// lk_mirror_kernel with NJ's own refusal: a cell of the strict upper triangle that is not finite (NaN, +inf, -inf) is tallied
__global__ void __launch_bounds__(kBlock)
nj_mirror_kernel(double* __restrict__ D, long long ld, int n, ClusterBad* __restrict__ bad) {
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
            if (!(v > -INFINITY && v < INFINITY)) { ++n_bad; const u64 at = (u64)a * (u64)n + (u64)b; first = at < first ? at : first; }
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

// THE SHAPE of a row sum (section 2l), for a workgroup of kNjSum lanes: lane l has added its columns l, l + kNjSum, ... in ascending
// order onto +0.0 (an inactive column and the diagonal add nothing) and hands in acc.  Each wave adds its 64 values in a butterfly
// over the lane strides 32, 16, 8, 4, 2, 1 (x + partner: the same bits in both lanes), and the 16 wave sums are added from wave 0
// upwards.  wsum: kNjSum / kWave doubles of LDS.  Every lane returns the sum
__device__ __forceinline__ double nj_row_sum(double acc, double* wsum) {
#pragma clang fp contract(off)
    for (int s = kWave / 2; s; s >>= 1) acc = acc + __shfl_xor(acc, s);
    __syncthreads();                                                           // (wsum may still be read from a call before)
    if (__lane_id() == 0) wsum[threadIdx.x / kWave] = acc;
    __syncthreads();
    double sum = wsum[0];
    for (int w = 1; w < kNjSum / kWave; ++w) sum = sum + wsum[w];
    return sum;
}

// R[s] of every row at the start (all columns active): one workgroup per row
__global__ void __launch_bounds__(kNjSum)
nj_rowsum_kernel(const double* __restrict__ D, long long ld, int n, double* __restrict__ R) {
#pragma clang fp contract(off)
    __shared__ double wsum[kNjSum / kWave];
    const int s = (int)blockIdx.x;
    const double* __restrict__ row = D + (long long)s * ld;
    double acc = 0.0;
    for (int k = (int)threadIdx.x; k < n; k += kNjSum)
        if (k != s) acc = acc + row[k];
    const double sum = nj_row_sum(acc, wsum);
    if (threadIdx.x == 0) R[s] = sum;
}

// q(a, c) of the definition; a NaN (inf - inf, once sums have overflowed) counts as +inf, so that a join always exists
__device__ __forceinline__ double nj_q(double rm2, double d, double ra, double rc) {
#pragma clang fp contract(off)
    const double p = rm2 * d;
    const double x = p - ra;
    const double q = x - rc;
    return q == q ? q : INFINITY;
}

// (q2, c2) replaces (q1, c1): c < 0 is "none yet"
__device__ __forceinline__ bool nj_better(double q1, int c1, double q2, int c2) { return c2 >= 0 && (c1 < 0 || q2 < q1 || (q2 == q1 && c2 < c1)); }

// kWide: ld even and the base 16-byte aligned, so every row is: two columns per load.  A lane visits its columns in ascending order,
// so inside a lane `<` alone keeps the smaller column among equal q.  grid: ceil(r / kNjRows)
template <bool kWide>
__global__ void __launch_bounds__(kBlock)
nj_scan_kernel(const double* __restrict__ D, long long ld, int n, int r, double rm2, const uint8_t* __restrict__ active, const double* __restrict__ R,
               const int* __restrict__ list, double* __restrict__ best_q, int* __restrict__ best_b) {
    const int pos0 = (int)blockIdx.x * kNjRows;
    int a[kNjRows];
    double ra[kNjRows], bq[kNjRows];
    int bb[kNjRows];
    const double* row[kNjRows];
#pragma unroll
    for (int i = 0; i < kNjRows; ++i) {
        a[i] = pos0 + i < r ? list[pos0 + i] : n;                              // (n: no column lies behind it; its row is never read)
        row[i] = D + (long long)(a[i] < n ? a[i] : 0) * ld;
        ra[i] = a[i] < n ? R[a[i]] : 0.0;
        bq[i] = 0.0;
        bb[i] = -1;
    }
    const int c0 = a[0] + 1;                                                   // (the list ascends: every row's columns lie at or behind this)
    if (kWide) {
#pragma unroll 2
        for (int c = (c0 & ~1) + 2 * (int)threadIdx.x; c < n; c += kNjScanCols) {
            if (c + 1 < n) {
                const double2 rc = *reinterpret_cast<const double2*>(R + c);                   // (c is even, R and active[] 16-byte aligned)
                const uint32_t on = *reinterpret_cast<const uint16_t*>(active + c);
#pragma unroll
                for (int i = 0; i < kNjRows; ++i) {
                    if (a[i] >= n) continue;
                    const double2 v = *reinterpret_cast<const double2*>(row[i] + c);
                    const double q0 = nj_q(rm2, v.x, ra[i], rc.x), q1 = nj_q(rm2, v.y, ra[i], rc.y);
                    if ((on & 0xFFu) && c > a[i] && (bb[i] < 0 || q0 < bq[i])) { bq[i] = q0; bb[i] = c; }
                    if ((on >> 8) && c + 1 > a[i] && (bb[i] < 0 || q1 < bq[i])) { bq[i] = q1; bb[i] = c + 1; }
                }
            } else {
                const double rc = R[c];
                const bool on = active[c] != 0;
#pragma unroll
                for (int i = 0; i < kNjRows; ++i) {
                    if (a[i] >= n) continue;
                    const double q = nj_q(rm2, row[i][c], ra[i], rc);
                    if (on && c > a[i] && (bb[i] < 0 || q < bq[i])) { bq[i] = q; bb[i] = c; }
                }
            }
        }
    } else {
#pragma unroll 2
        for (int c = c0 + (int)threadIdx.x; c < n; c += kBlock) {
            const double rc = R[c];
            const bool on = active[c] != 0;
#pragma unroll
            for (int i = 0; i < kNjRows; ++i) {
                if (a[i] >= n) continue;
                const double q = nj_q(rm2, row[i][c], ra[i], rc);
                if (on && c > a[i] && (bb[i] < 0 || q < bq[i])) { bq[i] = q; bb[i] = c; }
            }
        }
    }
    __shared__ double wq[kNjRows][kWavesPerBlock];
    __shared__ int wb[kNjRows][kWavesPerBlock];
#pragma unroll
    for (int i = 0; i < kNjRows; ++i) {
        for (int s = kWave / 2; s; s >>= 1) {
            const double oq = __shfl_xor(bq[i], s);
            const int ob = __shfl_xor(bb[i], s);
            if (nj_better(bq[i], bb[i], oq, ob)) { bq[i] = oq; bb[i] = ob; }
        }
        if (__lane_id() == 0) { wq[i][threadIdx.x / kWave] = bq[i]; wb[i][threadIdx.x / kWave] = bb[i]; }
    }
    __syncthreads();
    if (threadIdx.x < kNjRows && pos0 + (int)threadIdx.x < r) {
        const int i = (int)threadIdx.x;
        double q = wq[i][0];
        int b = wb[i][0];
        for (int w = 1; w < kWavesPerBlock; ++w)
            if (nj_better(q, b, wq[i][w], wb[i][w])) { q = wq[i][w]; b = wb[i][w]; }
        best_q[pos0 + i] = q;
        best_b[pos0 + i] = b;                                                  // (-1: the last active slot has no column behind it)
    }
}

// launched as one workgroup.  s: the join's number = where its record goes; r = n - s >= 2 active slots
__global__ void __launch_bounds__(kNjSum)
nj_pick_kernel(const double* __restrict__ D, long long ld, int n, int r, double rm2, int s, const uint8_t* __restrict__ active, double* __restrict__ R,
               const int* __restrict__ list, const double* __restrict__ best_q, const int* __restrict__ best_b, selhip_nj_join_t* __restrict__ joins,
               NjPick* __restrict__ pick) {
#pragma clang fp contract(off)
    __shared__ double wq[kNjSum / kWave];
    __shared__ int wa[kNjSum / kWave], wb[kNjSum / kWave];
    __shared__ double wsum[kNjSum / kWave];
    // the best row under (q, a, b); ba < 0 is "none yet"
    double bq = 0.0;
    int ba = -1, bb = -1;
    for (int pos = (int)threadIdx.x; pos < r; pos += kNjSum) {
        const int b = best_b[pos];
        if (b < 0) continue;
        const double q = best_q[pos];
        const int a = list[pos];
        if (ba < 0 || q < bq || (q == bq && a < ba)) { bq = q; ba = a; bb = b; }
    }
    for (int x = kWave / 2; x; x >>= 1) {
        const double oq = __shfl_xor(bq, x);
        const int oa = __shfl_xor(ba, x), ob = __shfl_xor(bb, x);
        if (oa >= 0 && (ba < 0 || oq < bq || (oq == bq && oa < ba))) { bq = oq; ba = oa; bb = ob; }
    }
    if (__lane_id() == 0) { wq[threadIdx.x / kWave] = bq; wa[threadIdx.x / kWave] = ba; wb[threadIdx.x / kWave] = bb; }
    __syncthreads();
    bq = wq[0]; ba = wa[0]; bb = wb[0];
    for (int w = 1; w < kNjSum / kWave; ++w)
        if (wa[w] >= 0 && (ba < 0 || wq[w] < bq || (wq[w] == bq && wa[w] < ba))) { bq = wq[w]; ba = wa[w]; bb = wb[w]; }
    if (ba < 0) return;                                                        // (r >= 2 active slots always give a pair: not reached)
    const int a = ba, b = bb;
    const double* __restrict__ row_a = D + (long long)a * ld;
    const double* __restrict__ row_b = D + (long long)b * ld;
    const double d = row_a[b];
    const double r_a = R[a], r_b = R[b];
    // the fresh sum of the new row, from the rows as they still are (the update's v, the same bits)
    double sum = 0.0;
    if (r > 2) {
        double acc = 0.0;
        for (int k = (int)threadIdx.x; k < n; k += kNjSum)
            if (active[k] && k != a && k != b) {
                const double t = row_a[k] + row_b[k];
                const double u = t - d;
                acc = acc + 0.5 * u;
            }
        sum = nj_row_sum(acc, wsum);                                           // (its barriers stand behind every lane's read of R[a])
    }
    if (threadIdx.x == 0) {
        const double half = 0.5 * d;
        double len_a = half;
        if (r > 2) {
            const double diff = r_a - r_b, den = 2.0 * rm2;
            len_a = half + diff / den;
        }
        const double len_b = r > 2 ? d - len_a : half;
        joins[s] = selhip_nj_join_t{a, b, len_a, len_b};
        pick->a = a; pick->b = b; pick->d = d;
        if (r > 2) R[a] = sum;
    }
}

// one lane per slot k, and per list position k: the new row's cell with its mirror and R[k]; b retired; list_out[0 .. r - 1) = list_in
// without b, in order.  In place: lane k alone reads [a][k], and row b is written by nobody
__global__ void __launch_bounds__(kBlock)
nj_update_kernel(double* D, long long ld, int n, int r, const NjPick* __restrict__ pick, uint8_t* __restrict__ active, double* __restrict__ R,
                 const int* __restrict__ list_in, int* __restrict__ list_out) {
#pragma clang fp contract(off)
    const int a = pick->a, b = pick->b;
    const double d = pick->d;
    double* const row_a = D + (long long)a * ld;
    const double* const row_b = D + (long long)b * ld;
    const int stride = (int)gridDim.x * kBlock;
    for (int k = (int)blockIdx.x * kBlock + (int)threadIdx.x; k < n; k += stride) {
        if (k < r - 1) {
            const int x = list_in[k];
            list_out[k] = x >= b ? list_in[k + 1] : x;
        }
        if (k == b) { active[k] = 0; continue; }
        if (k == a || !active[k]) continue;
        const double x = row_a[k], y = row_b[k];
        const double t = x + y;
        const double u = t - d;
        const double v = 0.5 * u;
        const double r1 = R[k] - x;
        const double r2 = r1 - y;
        R[k] = r2 + v;
        row_a[k] = v;
        D[(long long)k * ld + a] = v;
    }
}

}  // namespace

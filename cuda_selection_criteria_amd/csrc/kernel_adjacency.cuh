// kernel_adjacency.cuh -- the sparse adjacency (CSR) of a record list, built on the device (include/selection_hip.h section 2n):
// row offsets, the columns ascending inside each row, the values, entries with the same (row, column) merged into the one with the
// greatest value under kernel_topk.cuh's key order.
//   adj_count_kernel     entries per row: a record {i, k, v} with v >= min_value gives (row i, column k) and, in the symmetric form and
//                        with i != k, (row k, column i).  The tile rule of kernel_topk.cuh: one atomic per run of equal i inside a
//                        wave's tile, per-record atomics on the k side only
//   (rocprim::exclusive_scan of the counts: every row's segment start)
//   adj_scatter_kernel   (column, key(v)) of every entry into its row's segment: 12 bytes each in two arrays
//   the segmented sort   each segment ordered by (column ascending, key descending); an entry is KEPT iff it is the first of its
//                        column, the kept entries move to the front of the segment and their number is the row's kept count.
//                        Three kernels, one per class of segment length L, each of which takes only its own rows:
//     adj_sort_wave_kernel   L <= 64: one wave per row, one entry per lane in registers, a 21-step sorting network over the 96-bit
//                            composite with cross-lane moves; no LDS, no barrier, four rows per block.  A wave that meets a longer row
//                            appends it to the list of its class and goes on: the two kernels below walk those lists
//     adj_sort_block_kernel  64 < L <= kAdjLdsCap: one workgroup per row; the segment is staged once in LDS, sorted and compacted
//                            there, written back once
//     adj_sort_long_kernel   longer: one workgroup streams the segment into a 256-bin histogram of column * 256 / n_cols, scans it in
//                            LDS, scatters the entries bin by bin into a second scratch segment, and then sorts runs of consecutive
//                            bins that fit kAdjLdsCap together with the LDS routine; a single bin beyond kAdjLdsCap (one column range
//                            listed thousands of times) is sorted by the same workgroup through global memory -- correctness only
//   (rocprim::exclusive_scan of the kept counts: d_row_ptr)
//   adj_compact_kernel   one lane per kept entry: its row from d_row_ptr, its column and key^-1 = the value's bits to d_col / d_val
// The network.  Every sort here is the bitonic merge network in its one-direction form: the first step of a merge of blocks of k pairs
// t with t ^ (k - 1), the following steps pair t with t ^ j, j = k / 4 ... 1, and every compare-exchange moves the smaller composite to
// the smaller index.  Positions at or past L behave as entries greater than any real one and never move, so no padding is stored and
// a length that is no power of two costs nothing but the skipped pairs.
// Equal composites are equal entries, so the sorted segment, the kept set and every output are a function of the multiset of entries.
// No kernel waits for another workgroup.
#pragma once

namespace {

constexpr int kAdjLdsCap = 4096;                // longest segment sorted in LDS: 4 096 x 12 bytes = 48 KiB
constexpr int kAdjBlock = 512;                  // threads of the block and long kernels
constexpr int kAdjPer = kAdjLdsCap / kAdjBlock; // entries a thread compacts
constexpr int kAdjBins = 256;                   // column ranges a long row is split into
constexpr unsigned kAdjListBlocks = 1024;       // blocks of the block and long kernels; each strides over its class's list
// LDS of the block and long kernels: keys, columns, bin starts (one past the last), bin cursors, 8 wave totals and a counter --
// 50.1 KiB: three blocks stay resident in a CU's 160 KiB
constexpr size_t kAdjLdsBytes = (size_t)kAdjLdsCap * 12 + (kAdjBins + 1) * 4 + kAdjBins * 4 + 16 * 4;
static_assert(2 * kAdjLdsBytes <= 160 * 1024, "two sort blocks per CU");
static_assert(kAdjPer * kAdjBlock == kAdjLdsCap && (kAdjLdsCap & (kAdjLdsCap - 1)) == 0, "compaction and sort geometry");

// the two kinds of list: a pass's records, and a caller's entries with their values (none: 1.0 each)
struct AdjRecordList {
    const selhip_pair_t* p;                     // 16-byte records, 16-byte aligned
    __device__ __forceinline__ void get(u64 e, int* i, int* k, u64* bits) const {
        const uint4 w = reinterpret_cast<const uint4*>(p)[e];
        *i = (int)w.x; *k = (int)w.y; *bits = (u64)w.z | ((u64)w.w << 32);
    }
};
struct AdjPairList {
    const selhip_int2_t* p;
    const double* values;
    __device__ __forceinline__ void get(u64 e, int* i, int* k, u64* bits) const {
        const selhip_int2_t r = p[e];
        *i = r.x; *k = r.y;
        *bits = values ? (u64)__double_as_longlong(values[e]) : 0x3FF0000000000000ull;
    }
};

// is record (i, k, bits) an entry?  A rank out of range is tallied and is none; a value below the cut, or a NaN, is none
__device__ __forceinline__ bool adj_entry(int i, int k, u64 bits, u64 e, int n_rows, int n_cols, double min_value, ClusterBad* __restrict__ bad) {
    if ((uint32_t)i >= (uint32_t)n_rows || (uint32_t)k >= (uint32_t)n_cols) {
        atomicAdd(&bad->count, 1ull); atomicMin(&bad->index, e);
        return false;
    }
    return __longlong_as_double((long long)bits) >= min_value;
}

// words[0, n) = 0 and the two tallies (if any) empty: the one clearing launch of a chain, in place of a memset
__global__ __launch_bounds__(kBlock)
void adj_init_kernel(uint32_t* __restrict__ words, u64 n, ClusterBad* __restrict__ bad) {
    for (u64 t = (u64)blockIdx.x * kBlock + threadIdx.x; t < n; t += (u64)gridDim.x * kBlock) words[t] = 0;
    if (bad && blockIdx.x == 0 && threadIdx.x < 2) { bad[threadIdx.x].count = 0; bad[threadIdx.x].index = ~0ull; }
}

// cnt[n_rows]: entries per row, zero on entry.  SYM: n_rows == n_cols
template <class List, bool SYM>
__global__ __launch_bounds__(kBlock)
void adj_count_kernel(const List list, u64 n, int n_rows, int n_cols, double min_value, uint32_t* __restrict__ cnt, ClusterBad* __restrict__ bad) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    constexpr u64 tile = (u64)kTopkTile * kWave;
    for (u64 base = wave * tile; base < n; base += waves * tile) {
        int i0, k0; u64 b0;
        list.get(base, &i0, &k0, &b0);
        i0 = __builtin_amdgcn_readfirstlane(i0);
        uint32_t n0 = 0;
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const u64 j = base + (u64)t * kWave + lane;
            int i = -1, k = -1; u64 bits = 0;
            bool ok = false;
            if (j < n) { list.get(j, &i, &k, &bits); ok = adj_entry(i, k, bits, j, n_rows, n_cols, min_value, bad); }
            const bool same = ok && i == i0;
            n0 += (uint32_t)__popcll(__ballot(same));
            if (ok && !same) atomicAdd(&cnt[i], 1u);
            if constexpr (SYM) {
                if (ok && i != k) atomicAdd(&cnt[k], 1u);
            }
        }
        if (lane == 0 && n0) atomicAdd(&cnt[i0], n0);       // (n0 > 0: some lane's entry carries i0, so i0 is in range)
    }
}

// one slot of row r's segment, drawn from its fill cursor
__device__ __forceinline__ u64 adj_slot(const u64* __restrict__ off, uint32_t* __restrict__ cur, int r) { return off[r] + (u64)atomicAdd(&cur[r], 1u); }

__device__ __forceinline__ void adj_put(u64* __restrict__ seg_key, uint32_t* __restrict__ seg_col, u64 seg_cap, u64 pos, u64 key, uint32_t col) {
    if (pos < seg_cap) { seg_key[pos] = key; seg_col[pos] = col; }
}

// cur[n_rows]: fill cursors, zero on entry.  off[r] = start of row r's segment; seg_key / seg_col hold seg_cap entries, the scan's total
template <class List, bool SYM>
__global__ __launch_bounds__(kBlock)
void adj_scatter_kernel(const List list, u64 n, int n_rows, int n_cols, double min_value, const u64* __restrict__ off, uint32_t* __restrict__ cur,
                        u64* __restrict__ seg_key, uint32_t* __restrict__ seg_col, u64 seg_cap, ClusterBad* __restrict__ bad) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    constexpr u64 tile = (u64)kTopkTile * kWave;
    for (u64 base = wave * tile; base < n; base += waves * tile) {
        int ri[kTopkTile], rk[kTopkTile];
        u64 rb[kTopkTile], same_mask[kTopkTile];
        bool rok[kTopkTile];
        int i0, k0; u64 b0;
        list.get(base, &i0, &k0, &b0);
        i0 = __builtin_amdgcn_readfirstlane(i0);
        uint32_t n0 = 0;
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const u64 j = base + (u64)t * kWave + lane;
            ri[t] = -1; rk[t] = -1; rb[t] = 0; rok[t] = false;
            if (j < n) { list.get(j, &ri[t], &rk[t], &rb[t]); rok[t] = adj_entry(ri[t], rk[t], rb[t], j, n_rows, n_cols, min_value, bad); }
            same_mask[t] = __ballot(rok[t] && ri[t] == i0);
            n0 += (uint32_t)__popcll(same_mask[t]);
        }
        u64 at0 = 0;
        if (n0) {                                           // (wave-uniform; i0 is in range, see the count kernel)
            uint32_t c0 = 0;
            if (lane == 0) c0 = atomicAdd(&cur[i0], n0);
            at0 = off[i0] + (u64)(uint32_t)__builtin_amdgcn_readfirstlane((int)c0);
        }
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const u64 key = topk_key(rb[t]);
            if (rok[t]) {
                const u64 pos = ri[t] == i0 ? at0 + (u64)__popcll(same_mask[t] & ((1ull << lane) - 1ull)) : adj_slot(off, cur, ri[t]);
                adj_put(seg_key, seg_col, seg_cap, pos, key, (uint32_t)rk[t]);
                if constexpr (SYM) {
                    if (ri[t] != rk[t]) adj_put(seg_key, seg_col, seg_cap, adj_slot(off, cur, rk[t]), key, (uint32_t)ri[t]);
                }
            }
            at0 += (u64)__popcll(same_mask[t]);
        }
    }
}

// the composite order: column ascending, then key descending
__device__ __forceinline__ bool adj_before(uint32_t ca, u64 ka, uint32_t cb, u64 kb) { return ca < cb || (ca == cb && ka > kb); }

// ctl[0] / ctl[1]: rows in the block / long class; mid_list / long_list: their ranks, n_rows slots each
__global__ __launch_bounds__(kBlock)
void adj_sort_wave_kernel(const u64* __restrict__ off, int n_rows, u64* __restrict__ seg_key, uint32_t* __restrict__ seg_col, uint32_t* __restrict__ kept,
                          uint32_t* __restrict__ ctl, uint32_t* __restrict__ mid_list, uint32_t* __restrict__ long_list) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    for (u64 r = wave; r < (u64)n_rows; r += waves) {
        const u64 s0 = off[r], L = off[r + 1] - s0;
        if (L > (u64)kWave) {
            if (lane == 0) {
                const bool mid = L <= (u64)kAdjLdsCap;
                const uint32_t at = atomicAdd(&ctl[mid ? 0 : 1], 1u);
                if (at < (uint32_t)n_rows) (mid ? mid_list : long_list)[at] = (uint32_t)r;
            }
            continue;
        }
        const bool have = (u64)lane < L;
        uint32_t col = have ? seg_col[s0 + lane] : 0xFFFFFFFFu;
        u64 key = have ? seg_key[s0 + lane] : 0ull;
        // a compare-exchange with lane ^ mask; bit: the bit of the lane number that tells the pair's two lanes apart.  The smaller
        // index keeps the composite that comes first
        const auto step = [&](int mask, int bit) {
            const uint32_t oc = (uint32_t)__shfl_xor((int)col, mask, kWave);
            const u64 ok = (u64)__shfl_xor((long long)key, mask, kWave);
            const bool lower = (lane & bit) == 0;
            if (lower ? adj_before(oc, ok, col, key) : adj_before(col, key, oc, ok)) { col = oc; key = ok; }
        };
        if (L > 1) {                                        // (wave-uniform)
#pragma unroll
            for (int k = 2; k <= kWave; k <<= 1) {
                step(k - 1, k >> 1);
#pragma unroll
                for (int j = k >> 2; j > 0; j >>= 1) step(j, j);
            }
        }
        const uint32_t prev = (uint32_t)__shfl_up((int)col, 1, kWave);
        const bool keep = have && (lane == 0 || col != prev);
        const u64 km = __ballot(keep);
        if (keep) {
            const u64 pos = s0 + (u64)__popcll(km & ((1ull << lane) - 1ull));
            seg_col[pos] = col; seg_key[pos] = key;
        }
        if (lane == 0) kept[r] = (uint32_t)__popcll(km);
    }
}

// (skey, scol)[0, L) in LDS, L <= kAdjLdsCap: sorted by the composite, then the kept entries moved to the front in order.  Returns their
// number to every thread.  wsum: 9 words of LDS.  Called by all kAdjBlock threads; the arrays are complete before the call (a barrier
// stands in front of it) and settled behind it
__device__ __forceinline__ uint32_t adj_lds_sort_compact(u64* skey, uint32_t* scol, uint32_t L, uint32_t* wsum) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    uint32_t n = 1;
    while (n < L) n <<= 1;
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            const bool first = j == (k >> 1);
            for (uint32_t q = tid; q < (n >> 1); q += kAdjBlock) {
                const uint32_t lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const uint32_t hi = first ? lo ^ (k - 1) : lo | j;
                if (hi < L) {
                    const u64 ka = skey[lo], kb = skey[hi];
                    const uint32_t ca = scol[lo], cb = scol[hi];
                    if (adj_before(cb, kb, ca, ka)) { skey[lo] = kb; scol[lo] = cb; skey[hi] = ka; scol[hi] = ca; }
                }
            }
            __syncthreads();
        }
    }
    // thread t owns the entries [kAdjPer t, kAdjPer t + kAdjPer)
    u64 rk[kAdjPer];
    uint32_t rc[kAdjPer];
    const uint32_t e0 = (uint32_t)tid * kAdjPer;
    uint32_t prev = e0 > 0 && e0 <= L ? scol[e0 - 1] : 0xFFFFFFFFu, mine = 0, flags = 0;
#pragma unroll
    for (int u = 0; u < kAdjPer; ++u) {
        const uint32_t e = e0 + u;
        rc[u] = 0; rk[u] = 0;
        if (e < L) {
            rc[u] = scol[e]; rk[u] = skey[e];
            if (e == 0 || rc[u] != prev) { flags |= 1u << u; ++mine; }
            prev = rc[u];
        }
    }
    uint32_t inc = mine;
#pragma unroll
    for (int w = 1; w < kWave; w <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, w, kWave); if (lane >= w) inc += o; }
    if (lane == kWave - 1) wsum[wave] = inc;
    __syncthreads();                                        // every entry is in registers, the wave totals are written
    uint32_t at = inc - mine, total = 0;
#pragma unroll
    for (int w = 0; w < kAdjBlock / kWave; ++w) { const uint32_t s = wsum[w]; if (w < wave) at += s; total += s; }
#pragma unroll
    for (int u = 0; u < kAdjPer; ++u)
        if ((flags >> u) & 1u) { scol[at] = rc[u]; skey[at] = rk[u]; ++at; }
    __syncthreads();
    return total;
}

__global__ __launch_bounds__(kAdjBlock)
void adj_sort_block_kernel(const u64* __restrict__ off, u64* __restrict__ seg_key, uint32_t* __restrict__ seg_col, uint32_t* __restrict__ kept,
                           const uint32_t* __restrict__ ctl, const uint32_t* __restrict__ mid_list, int n_rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char adj_smem[];
    u64* skey = reinterpret_cast<u64*>(adj_smem);                               // [kAdjLdsCap]
    uint32_t* scol = reinterpret_cast<uint32_t*>(skey + kAdjLdsCap);            // [kAdjLdsCap]
    uint32_t* wsum = scol + kAdjLdsCap + 2 * kAdjBins + 1;                      // [16]
    const int tid = threadIdx.x;
    const uint32_t rows = ctl[0] < (uint32_t)n_rows ? ctl[0] : (uint32_t)n_rows;
    for (uint32_t u = blockIdx.x; u < rows; u += gridDim.x) {
        const uint32_t r = mid_list[u];
        if (r >= (uint32_t)n_rows) continue;
        const u64 s0 = off[r];
        const u64 L64 = off[r + 1] - s0;
        const uint32_t L = L64 < (u64)kAdjLdsCap ? (uint32_t)L64 : (uint32_t)kAdjLdsCap;
        for (uint32_t t = tid; t < L; t += kAdjBlock) { skey[t] = seg_key[s0 + t]; scol[t] = seg_col[s0 + t]; }
        __syncthreads();
        const uint32_t total = adj_lds_sort_compact(skey, scol, L, wsum);
        for (uint32_t t = tid; t < total; t += kAdjBlock) { seg_key[s0 + t] = skey[t]; seg_col[s0 + t] = scol[t]; }
        if (tid == 0) kept[r] = total;
        __syncthreads();
    }
}

// the bin of a column: column * 256 / n_cols, ascending with the column
__device__ __forceinline__ uint32_t adj_bin(uint32_t col, int n_cols) { return (uint32_t)(((u64)col * kAdjBins) / (u64)(uint32_t)n_cols); }

// (key, col)[0, L) in global memory sorted by the composite by the whole workgroup: the same network, a barrier per step
__device__ __forceinline__ void adj_global_sort(u64* key, uint32_t* col, u64 L) {
    u64 n = 1;
    while (n < L) n <<= 1;
    for (u64 k = 2; k <= n; k <<= 1) {
        for (u64 j = k >> 1; j > 0; j >>= 1) {
            const bool first = j == (k >> 1);
            for (u64 q = threadIdx.x; q < (n >> 1); q += kAdjBlock) {
                const u64 lo = ((q & ~(j - 1)) << 1) | (q & (j - 1));
                const u64 hi = first ? lo ^ (k - 1) : lo | j;
                if (hi < L) {
                    const u64 ka = key[lo], kb = key[hi];
                    const uint32_t ca = col[lo], cb = col[hi];
                    if (adj_before(cb, kb, ca, ka)) { key[lo] = kb; col[lo] = cb; key[hi] = ka; col[hi] = ca; }
                }
            }
            __syncthreads();
        }
    }
}

// seg2_key / seg2_col: a second scratch of the segments' size, written and read inside a long row's own range only
__global__ __launch_bounds__(kAdjBlock)
void adj_sort_long_kernel(const u64* __restrict__ off, int n_cols, u64* seg_key, uint32_t* seg_col, u64* seg2_key, uint32_t* seg2_col, uint32_t* __restrict__ kept, const uint32_t* __restrict__ ctl,
                          const uint32_t* __restrict__ long_list, int n_rows) {
    extern __shared__ __attribute__((aligned(16))) unsigned char adj_smem[];
    u64* skey = reinterpret_cast<u64*>(adj_smem);                               // [kAdjLdsCap]
    uint32_t* scol = reinterpret_cast<uint32_t*>(skey + kAdjLdsCap);            // [kAdjLdsCap]
    uint32_t* bstart = scol + kAdjLdsCap;                                       // [kAdjBins + 1]
    uint32_t* bcur = bstart + kAdjBins + 1;                                     // [kAdjBins]
    uint32_t* wsum = bcur + kAdjBins;                                           // [16]
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const uint32_t rows = ctl[1] < (uint32_t)n_rows ? ctl[1] : (uint32_t)n_rows;
    for (uint32_t u = blockIdx.x; u < rows; u += gridDim.x) {
        const uint32_t r = long_list[u];
        if (r >= (uint32_t)n_rows) continue;
        const u64 s0 = off[r], L64 = off[r + 1] - s0;
        if (L64 > 0xFFFFFFFFull) continue;                  // (the host admits fewer entries than that in all)
        const uint32_t L = (uint32_t)L64;
        u64* const k1 = seg_key + s0; uint32_t* const c1 = seg_col + s0;       // the row's segment, and its twin
        u64* const k2 = seg2_key + s0; uint32_t* const c2 = seg2_col + s0;
        if (tid < kAdjBins) { bcur[tid] = 0; bstart[tid] = 0; }
        __syncthreads();
        for (uint32_t t = tid; t < L; t += kAdjBlock) atomicAdd(&bstart[adj_bin(c1[t], n_cols) & (kAdjBins - 1)], 1u);
        __syncthreads();
        if (wave == 0) {
            // lane l owns bins 4l .. 4l + 3; exclusive scan across the lanes
            uint32_t h[4], s = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) { h[b] = bstart[4 * lane + b]; s += h[b]; }
            uint32_t inc = s;
#pragma unroll
            for (int w = 1; w < kWave; w <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, w, kWave); if (lane >= w) inc += o; }
            uint32_t at = inc - s;
#pragma unroll
            for (int b = 0; b < 4; ++b) { bstart[4 * lane + b] = at; at += h[b]; }
            if (lane == kWave - 1) bstart[kAdjBins] = at;
        }
        __syncthreads();
        for (uint32_t t = tid; t < L; t += kAdjBlock) {
            const uint32_t col = c1[t], b = adj_bin(col, n_cols) & (kAdjBins - 1);
            const uint32_t pos = bstart[b] + atomicAdd(&bcur[b], 1u);
            if (pos < L) { k2[pos] = k1[t]; c2[pos] = col; }
        }
        __syncthreads();
        // runs of consecutive bins that fit the LDS together, in column order; the kept entries go back to the segment's front
        uint32_t row_kept = 0;
        for (int b0 = 0; b0 < kAdjBins;) {
            int b1 = b0 + 1;
            const uint32_t p0 = bstart[b0];
            while (b1 < kAdjBins && bstart[b1 + 1] - p0 <= (uint32_t)kAdjLdsCap) ++b1;
            const uint32_t p1 = bstart[b1] < L ? bstart[b1] : L, len = p1 > p0 ? p1 - p0 : 0;
            if (len == 0) { b0 = b1; continue; }
            if (len <= (uint32_t)kAdjLdsCap) {
                for (uint32_t t = tid; t < len; t += kAdjBlock) { skey[t] = k2[p0 + t]; scol[t] = c2[p0 + t]; }
                __syncthreads();
                const uint32_t total = adj_lds_sort_compact(skey, scol, len, wsum);
                for (uint32_t t = tid; t < total; t += kAdjBlock) { k1[row_kept + t] = skey[t]; c1[row_kept + t] = scol[t]; }
                row_kept += total;
                __syncthreads();
            } else {
                // one bin beyond the LDS: sorted where it lies, then compacted in chunks of one entry per thread
                adj_global_sort(k2 + p0, c2 + p0, len);
                for (uint32_t base = 0; base < len; base += kAdjBlock) {
                    const uint32_t t = base + tid;
                    uint32_t col = 0; u64 key = 0;
                    bool keep = false;
                    if (t < len) { col = c2[p0 + t]; key = k2[p0 + t]; keep = t == 0 || c2[p0 + t - 1] != col; }
                    const u64 km = __ballot(keep);
                    if (lane == 0) wsum[wave] = (uint32_t)__popcll(km);
                    __syncthreads();
                    uint32_t at = row_kept + (uint32_t)__popcll(km & ((1ull << lane) - 1ull)), total = 0;
#pragma unroll
                    for (int w = 0; w < kAdjBlock / kWave; ++w) { const uint32_t s = wsum[w]; if (w < wave) at += s; total += s; }
                    if (keep) { k1[at] = key; c1[at] = col; }
                    row_kept += total;
                    __syncthreads();
                }
            }
            b0 = b1;
        }
        if (tid == 0) kept[r] = row_kept;
        __syncthreads();
    }
}

// the row of output j: the r with row_ptr[r] <= j < row_ptr[r + 1], searched in [lo, hi]
__device__ __forceinline__ int adj_row_of(const int64_t* __restrict__ row_ptr, int lo, int hi, int64_t j) {
    while (lo < hi) {
        const int mid = lo + (hi - lo + 1) / 2;
        if (row_ptr[mid] <= j) lo = mid; else hi = mid - 1;
    }
    return lo;
}

// one lane per kept entry.  A wave's 64 outputs mostly lie in one row or two: the rows of its first and last output bound every
// lane's search
__global__ __launch_bounds__(kBlock)
void adj_compact_kernel(const int64_t* __restrict__ row_ptr, int n_rows, const u64* __restrict__ off, const u64* __restrict__ seg_key,
                        const uint32_t* __restrict__ seg_col, u64 seg_cap, int64_t nnz, int32_t* __restrict__ d_col, double* __restrict__ d_val) {
    const int lane = threadIdx.x & (kWave - 1);
    const int64_t stride = (int64_t)gridDim.x * kBlock;
    for (int64_t j0 = ((int64_t)blockIdx.x * kBlock + threadIdx.x) - lane; j0 < nnz; j0 += stride) {
        const int64_t j = j0 + lane, jl = j0 + kWave - 1 < nnz - 1 ? j0 + kWave - 1 : nnz - 1;
        const int rf = adj_row_of(row_ptr, 0, n_rows - 1, j0);
        const int rl = adj_row_of(row_ptr, rf, n_rows - 1, jl);
        if (j < nnz) {
            const int r = adj_row_of(row_ptr, rf, rl, j);
            const u64 src = off[r] + (u64)(j - row_ptr[r]);
            if (src < seg_cap) {
                d_col[j] = (int32_t)seg_col[src];
                if (d_val) d_val[j] = __longlong_as_double((long long)topk_unkey(seg_key[src]));
            }
        }
    }
}

}  // namespace

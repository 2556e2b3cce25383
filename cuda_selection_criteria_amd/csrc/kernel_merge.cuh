// kernel_merge.cuh -- sketches merged by group (selhip_merge_sketches, selhip_ctx_merge_groups): one union sketch per group id.
// Part of libselhip.so; included by selection_kernels.hip only.
//
// THE TWO IDENTITIES.  An HLL register's index and rank are functions of the hash alone, so the sketch of a union of k-mer sets is the
// element-wise MAXIMUM of the members' registers (main and auxiliary sketches alike).  A SuperMinHash bucket is the minimum over all
// elements and steps of the values offered to it (kernel_sketch.cuh; the running bound only skips offers that cannot win), so the
// sketch of a union is the element-wise unsigned MINIMUM of the 64-bit buckets; an empty bucket stays ~0.  Both are exact: a merged row
// is bit for bit the row the builder writes for the members' records concatenated.
//
// THE DECOMPOSITION.  A counting sort groups the members (merge_count_kernel: members per group and the check of the ids; one exclusive
// scan of a packed u64 per level; merge_scatter_kernel).  merge_reduce_kernel then is a segmented reduction over rows that lie in HBM:
// a work item is one OUTPUT row x one 16-byte column of it, a lane per item, so the lanes of a wave read 1 KiB of a row side by side
// (rows of less than 1 KiB: a wave spans several rows), kMergeLoads member rows in flight per lane, the running value in registers, one
// store per item.  No item loops over more than SELHIP_MERGE_SEGMENT (S) rows: a group of c members has max(1, ceil(c / S)) output rows
// at a level; while some group has more than one, the output rows are partial sketches in scratch, in group order, and the next level
// reduces them the same way (maximum and minimum are associative) with the identity as member order.  The last level has one row per
// group and writes the caller's arrays.  No kernel waits for another; the only atomics are the counting sort's.
#pragma once

namespace {

constexpr int kMergeSegment = SELHIP_MERGE_SEGMENT;
constexpr int kMergeLoads = 4;             // member rows in flight per lane (16 B each), as kFoldLoads
constexpr unsigned kMergeMaxBlocks = 1u << 18;
constexpr int kMergeMaxLevels = 6;         // n < 2^31 members: S^6 >= 2^31 for S >= 36
static_assert(kMergeSegment >= 36 && kMergeSegment <= 4096, "SELHIP_MERGE_SEGMENT: kMergeMaxLevels levels must reduce 2^31 - 1 members");

enum MergeOp { kMergeMaxU8 = 0, kMergeMinU64 = 1 };

// what merge_count_kernel found: ids outside [-1, G) (their number, and ~(the smallest index of one): zero-initialised), the fullest group
struct MergeInfo {
    u64 bad_count, bad_index_inv;
    uint32_t max_cnt, pad;
};

__device__ __forceinline__ uint32_t merge_pk_max_u16(uint32_t a, uint32_t b) {
    typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_elementwise_max(__builtin_bit_cast(u16x2, a), __builtin_bit_cast(u16x2, b)));
}

// the running value of one 16-byte column.  u8 maximum: the even and the odd bytes of every dword as two registers of 16-bit fields
// (x & 0x00FF00FF, x & 0xFF00FF00 -- a byte in the high half of its field orders as it does in the low half), v_pk_max_u16 on each:
// exact for every byte value 0 .. 255.  u64 minimum: the two buckets of the column.
template <int OP> struct MergeAcc;
template <> struct MergeAcc<kMergeMaxU8> {
    uint32_t e[4], o[4];
    __device__ __forceinline__ void init() {
#pragma unroll
        for (int q = 0; q < 4; ++q) { e[q] = 0u; o[q] = 0u; }
    }
    __device__ __forceinline__ void add(const uint4& w) {
        const uint32_t dw[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            e[q] = merge_pk_max_u16(e[q], dw[q] & 0x00FF00FFu);
            o[q] = merge_pk_max_u16(o[q], dw[q] & 0xFF00FF00u);
        }
    }
    __device__ __forceinline__ uint4 get() const { return make_uint4(e[0] | o[0], e[1] | o[1], e[2] | o[2], e[3] | o[3]); }
    template <class VecT> static __device__ __forceinline__ VecT identity() { return make_uint4(0u, 0u, 0u, 0u); }
};
template <> struct MergeAcc<kMergeMinU64> {
    u64 a, b;
    __device__ __forceinline__ void init() { a = ~0ull; b = ~0ull; }
    __device__ __forceinline__ void add(const uint4& w) {
        const u64 x = (u64)w.x | ((u64)w.y << 32), y = (u64)w.z | ((u64)w.w << 32);
        a = x < a ? x : a;
        b = y < b ? y : b;
    }
    __device__ __forceinline__ void add(u64 x) { a = x < a ? x : a; }
    __device__ __forceinline__ uint4 get() const { return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32)); }
    __device__ __forceinline__ void get(u64* x) const { *x = a; }
    __device__ __forceinline__ void get(uint4* x) const { *x = get(); }
    template <class VecT> static __device__ __forceinline__ VecT identity() {
        if constexpr (sizeof(VecT) == 16) return make_uint4(~0u, ~0u, ~0u, ~0u); else return ~0ull;
    }
};

// The counting sort's atomics, aggregated per wave: the lanes that hold the group of the first lane still to be served are served by
// ONE atomic of their number, kMergeLeaders times over; what is left goes lane by lane.  One group of n members is otherwise n atomics on
// one address, which a single address takes at some 90 per microsecond (common.cuh: WaveAppender) -- the giant group of cfg3 0.11 ms per
// kernel; ids in random order pay two ballots for nothing.  Returns the value of `op(&cnt[g], lanes served)` of the lane's atomic and the
// lane's place among the lanes served by it through *place; valid lanes only (the others return 0).
constexpr int kMergeLeaders = 2;

template <class Op>
__device__ __forceinline__ int merge_wave_atomic(bool valid, int g, int* __restrict__ cnt, Op op, int* place) {
    const int lane = threadIdx.x & (kWave - 1);
    u64 todo = __ballot(valid);
    int base = 0;
    *place = 0;
    for (int round = 0; round < kMergeLeaders && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const int g_lead = __shfl(g, leader, kWave);
        const u64 same = __ballot(valid && g == g_lead) & todo;
        int got = 0;
        if (lane == leader) got = op(&cnt[g_lead], (int)__popcll(same));
        got = __shfl(got, leader, kWave);
        if ((same >> lane) & 1ull) { base = got; *place = (int)__popcll(same & ((1ull << lane) - 1ull)); }
        todo &= ~same;
    }
    if ((todo >> lane) & 1ull) base = op(&cnt[g], 1);
    return base;
}

// members per group.  An id outside [-1, G) is tallied in info and counted nowhere: nothing downstream indexes with it
__global__ __launch_bounds__(kBlock) void merge_count_kernel(const int* __restrict__ group, long long n, int n_groups, int* __restrict__ cnt,
                                                             MergeInfo* __restrict__ info) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i0 = (long long)blockIdx.x * kBlock; i0 < n; i0 += stride) {          // (block-uniform: the ballots see whole waves)
        const long long i = i0 + threadIdx.x;
        const int g = i < n ? group[i] : -1;
        const bool valid = (unsigned)g < (unsigned)n_groups;
        if (g != -1 && !valid) {
            atomicAdd(&info->bad_count, 1ull);
            atomicMax(&info->bad_index_inv, ~(u64)i);
        }
        int place;
        (void)merge_wave_atomic(valid, g, cnt, [](int* a, int k) { return atomicAdd(a, k); }, &place);
    }
}

// one level's scan input: pk[g] = members << 32 | output rows, output rows = max(1, ceil(members / S)); pk[G] = 0, where the exclusive
// scan leaves the totals.  Level 0 counts members in cnt[]; a later level's members are the previous level's output rows (prev = its scan)
__global__ __launch_bounds__(kBlock) void merge_pack_kernel(const int* __restrict__ cnt, const u64* __restrict__ prev, int n_groups,
                                                            u64* __restrict__ pk, MergeInfo* __restrict__ info) {
    const long long g = (long long)blockIdx.x * kBlock + threadIdx.x;
    uint32_t c = 0;
    if (g < n_groups) {
        c = prev ? (uint32_t)prev[g + 1] - (uint32_t)prev[g] : (uint32_t)cnt[g];
        const uint32_t rows = c ? (c + (uint32_t)kMergeSegment - 1u) / (uint32_t)kMergeSegment : 1u;
        pk[g] = ((u64)c << 32) | rows;
    } else if (g == n_groups) {
        pk[g] = 0;
    }
    if (!prev) {
        for (int s = kWave / 2; s > 0; s >>= 1) c = max(c, (uint32_t)__shfl_xor((int)c, s, kWave));
        if ((threadIdx.x & (kWave - 1)) == 0 && c) atomicMax(&info->max_cnt, c);
    }
}

// the members in group order: order[member offset of g ..] = the members of g, in any order (cnt[] counts down to zero)
__global__ __launch_bounds__(kBlock) void merge_scatter_kernel(const int* __restrict__ group, long long n, int n_groups, int* __restrict__ cnt,
                                                               const u64* __restrict__ scan, int* __restrict__ order) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long i0 = (long long)blockIdx.x * kBlock; i0 < n; i0 += stride) {          // (block-uniform, as above)
        const long long i = i0 + threadIdx.x;
        const int g = i < n ? group[i] : -1;
        const bool valid = (unsigned)g < (unsigned)n_groups;
        int place;
        const int left = merge_wave_atomic(valid, g, cnt, [](int* a, int k) { return atomicSub(a, k); }, &place) - place;
        if (valid && left > 0) order[(uint32_t)(scan[g] >> 32) + (uint32_t)(left - 1)] = (int)i;
    }
}

// rows[.][V] -> out[R][V], V elements of VecT per row; R = the scan's total of output rows.  Output row r of group g, its s-th, reduces the
// members order[lo .. hi), lo = offset(g) + s S, hi = min(lo + S, offset(g + 1)); order NULL = the identity (a later level's members are
// the previous level's rows, in group order).  one_row_per_group: R == G, so g = r; else g is searched in the row offsets.
// v_shift >= 0: V = 1 << v_shift.  Any grid.
template <int OP, class VecT>
__global__ __launch_bounds__(kBlock) void merge_reduce_kernel(const VecT* __restrict__ rows, const int* __restrict__ order, const u64* __restrict__ scan,
                                                              int n_groups, int one_row_per_group, u64 V, int v_shift, VecT* __restrict__ out) {
    const u64 R = (uint32_t)scan[n_groups];
    const u64 items = R * V, stride = (u64)gridDim.x * kBlock;
    for (u64 q = (u64)blockIdx.x * kBlock + threadIdx.x; q < items; q += stride) {
        const u64 r = v_shift >= 0 ? q >> v_shift : q / V;
        const u64 v = q - r * V;
        uint32_t g = (uint32_t)r;
        if (!one_row_per_group) {
            uint32_t lo_g = 0, hi_g = (uint32_t)n_groups;                      // the last g with row offset <= r (offsets ascend strictly)
            while (hi_g - lo_g > 1) {
                const uint32_t mid = lo_g + (hi_g - lo_g) / 2;
                if ((uint32_t)scan[mid] <= (uint32_t)r) lo_g = mid; else hi_g = mid;
            }
            g = lo_g;
        }
        const u64 a = scan[g], b = scan[g + 1];
        const uint32_t lo = (uint32_t)(a >> 32) + ((uint32_t)r - (uint32_t)a) * (uint32_t)kMergeSegment;
        const uint32_t end = (uint32_t)(b >> 32);
        const uint32_t hi = end - lo > (uint32_t)kMergeSegment ? lo + (uint32_t)kMergeSegment : end;
        MergeAcc<OP> acc;
        acc.init();
        for (uint32_t j = lo; j < hi; j += kMergeLoads) {
            VecT w[kMergeLoads];
#pragma unroll
            for (int k = 0; k < kMergeLoads; ++k) {
                if (j + k < hi) {
                    const u64 row = order ? (u64)(uint32_t)order[j + k] : (u64)(j + k);
                    w[k] = rows[row * V + v];
                } else {
                    w[k] = MergeAcc<OP>::template identity<VecT>();
                }
            }
#pragma unroll
            for (int k = 0; k < kMergeLoads; ++k) acc.add(w[k]);
        }
        VecT res;
        if constexpr (OP == kMergeMinU64) acc.get(&res); else res = acc.get();
        out[q] = res;
    }
}

template <int OP, class VecT>
hipError_t launch_merge_reduce_as(hipStream_t st, const void* rows, const int* order, const u64* scan, int n_groups, u64 out_rows, bool one_row_per_group,
                                  size_t row_bytes, void* out) {
    const u64 V = row_bytes / sizeof(VecT), items = out_rows * V;
    if (!items) return hipSuccess;
    int v_shift = -1;
    if ((V & (V - 1)) == 0) { v_shift = 0; while (((u64)1 << v_shift) < V) ++v_shift; }
    const unsigned grid = (unsigned)std::min<u64>((items + kBlock - 1) / kBlock, kMergeMaxBlocks);
    hipLaunchKernelGGL((merge_reduce_kernel<OP, VecT>), dim3(grid), dim3(kBlock), 0, st, (const VecT*)rows, order, scan, n_groups, one_row_per_group ? 1 : 0,
                       V, v_shift, (VecT*)out);
    return hipGetLastError();
}

// one level of one sketch kind.  HLL rows are whole 16-byte vectors (p >= 4).  SuperMinHash rows take the 16-byte path when m is even and
// both arrays are 16-byte aligned, else the plain 8-byte one (m = 1, odd m, a caller's 8-byte aligned array)
hipError_t launch_merge_reduce(hipStream_t st, int op, const void* rows, const int* order, const u64* scan, int n_groups, u64 out_rows,
                               bool one_row_per_group, size_t row_bytes, void* out) {
    if (op == kMergeMaxU8) return launch_merge_reduce_as<kMergeMaxU8, uint4>(st, rows, order, scan, n_groups, out_rows, one_row_per_group, row_bytes, out);
    if (row_bytes % 16 == 0 && !((uintptr_t)rows & 15) && !((uintptr_t)out & 15))
        return launch_merge_reduce_as<kMergeMinU64, uint4>(st, rows, order, scan, n_groups, out_rows, one_row_per_group, row_bytes, out);
    return launch_merge_reduce_as<kMergeMinU64, u64>(st, rows, order, scan, n_groups, out_rows, one_row_per_group, row_bytes, out);
}

}  // namespace

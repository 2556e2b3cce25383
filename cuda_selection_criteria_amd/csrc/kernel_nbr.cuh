// kernel_nbr.cuh -- top-k of an all-pairs pass (include/selection_hip.h section 2, selhip_ctx_set_allpairs_topk): every record
// {i, k, J}, i < k, of the pass belongs to BOTH genomes' lists -- {owner i, partner k, J} and {owner k, partner i, J} -- and every
// genome keeps its K best partners, ranked as kernel_topk.cuh ranks a query's records (key(J) descending, partner ascending).
//   nbr_count_kernel     directed records per genome: one count for a record's i, one for its k
//   (rocprim::exclusive_scan of the packed counts, TopkPack: low word = a genome's segment start, high word = its output start)
//   nbr_scatter_kernel   (key(J), partner) of both directed records into their owners' segments: 12 bytes per directed record
//   topk_select_kernel   (kernel_topk.cuh, as it is) one block per genome: radix select of the K best, bitonic sort, records written
// The i side arrives clustered by i (bucketed by row where stage 2 groups, row by row from the dense kernel) and is grouped as
// kernel_topk.cuh groups a query's records: a wave takes kTopkTile * 64 consecutive records and covers everything that carries its
// first record's i with ONE atomic.  The k side arrives in no order; it takes one atomic per record (no return value in the count
// kernel, a returned cursor in the scatter kernel).  Along a row the k are ascending, mostly consecutive, so a wave's 64 atomics fall
// on few cache lines; only a genome that is the larger member of very many pairs (a hub fed from the k side) makes one word hot.
#pragma once

namespace {

__global__ __launch_bounds__(kBlock)
void nbr_count_kernel(const selhip_pair_t* __restrict__ res, u64 n, int n_g, uint32_t* __restrict__ cnt) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    constexpr u64 tile = (u64)kTopkTile * kWave;
    for (u64 base = wave * tile; base < n; base += waves * tile) {
        const int i0 = __builtin_amdgcn_readfirstlane(res[base].i);
        uint32_t n0 = 0;
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const u64 j = base + (u64)t * kWave + lane;
            const int i = j < n ? res[j].i : -1;
            const int k = j < n ? res[j].k : -1;
            const bool same = i == i0;
            n0 += (uint32_t)__popcll(__ballot(same));
            if (!same && (unsigned)i < (unsigned)n_g) atomicAdd(&cnt[i], 1u);
            if ((unsigned)k < (unsigned)n_g) atomicAdd(&cnt[k], 1u);
        }
        if (lane == 0 && (unsigned)i0 < (unsigned)n_g) atomicAdd(&cnt[i0], n0);
    }
}

// cur[n_g]: fill cursors, zero on entry (one per genome: both sides draw from it).  off[g] low word = start of genome g's segment;
// seg_key / seg_val hold seg_cap = 2 n entries
__global__ __launch_bounds__(kBlock)
void nbr_scatter_kernel(const selhip_pair_t* __restrict__ res, u64 n, int n_g, const u64* __restrict__ off, uint32_t* __restrict__ cur,
                        u64* __restrict__ seg_key, uint32_t* __restrict__ seg_val, u64 seg_cap) {
    const int lane = threadIdx.x & (kWave - 1);
    const u64 wave = ((u64)blockIdx.x * kBlock + threadIdx.x) / kWave, waves = (u64)gridDim.x * kWavesPerBlock;
    constexpr u64 tile = (u64)kTopkTile * kWave;
    const uint4* __restrict__ res4 = reinterpret_cast<const uint4*>(res);       // {i, k, J low, J high}
    static_assert(sizeof(selhip_pair_t) == 16, "records are read as one 16-byte word");
    for (u64 base = wave * tile; base < n; base += waves * tile) {
        uint4 rec[kTopkTile];
        u64 same_mask[kTopkTile];
        const int i0 = __builtin_amdgcn_readfirstlane((int)res4[base].x);
        uint32_t n0 = 0;
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const u64 j = base + (u64)t * kWave + lane;
            rec[t] = j < n ? res4[j] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);
            same_mask[t] = __ballot((int)rec[t].x == i0);
            n0 += (uint32_t)__popcll(same_mask[t]);
        }
        const bool ok0 = (unsigned)i0 < (unsigned)n_g;
        uint32_t at0 = 0;
        if (lane == 0 && ok0) at0 = atomicAdd(&cur[i0], n0);
        at0 = (uint32_t)__builtin_amdgcn_readfirstlane((int)at0);
        if (ok0) at0 += (uint32_t)off[i0];
#pragma unroll
        for (int t = 0; t < kTopkTile; ++t) {
            const int i = (int)rec[t].x, k = (int)rec[t].y;
            const u64 key = topk_key((u64)rec[t].z | ((u64)rec[t].w << 32));
            // owner i, partner k
            u64 pos = seg_cap;
            if (i == i0) {
                if (ok0) pos = (u64)at0 + (u64)__popcll(same_mask[t] & ((1ull << lane) - 1ull));
            } else if ((unsigned)i < (unsigned)n_g) {
                pos = (u64)(uint32_t)off[i] + (u64)atomicAdd(&cur[i], 1u);
            }
            at0 += (uint32_t)__popcll(same_mask[t]);
            if (pos < seg_cap) { seg_key[pos] = key; seg_val[pos] = (uint32_t)k; }
            // owner k, partner i
            if ((unsigned)k < (unsigned)n_g) {
                const u64 posk = (u64)(uint32_t)off[k] + (u64)atomicAdd(&cur[k], 1u);
                if (posk < seg_cap) { seg_key[posk] = key; seg_val[posk] = (uint32_t)i; }
            }
        }
    }
}

}  // namespace

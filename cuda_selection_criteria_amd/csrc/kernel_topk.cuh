// kernel_topk.cuh -- the device-side top-k of a pass: every owner keeps its K best records, ranked by (J descending in the IEEE total
// order, partner ascending), and the list comes out in ranked order: owner ascending, then that ranking.  Two forms of one machinery:
//   query pass (include/selection_hip.h section 2b, selhip_ctx_set_query_topk): of the records {i = query rank, k = database rank, J}
//     every query i keeps its K best k -- one owner per record (BOTH = false);
//   all-pairs pass (section 2, selhip_ctx_set_allpairs_topk): every record {i, k, J}, i < k, belongs to BOTH genomes' lists --
//     {owner i, partner k, J} and {owner k, partner i, J} -- and every genome keeps its K best partners (BOTH = true).
//   topk_count_kernel    records per owner (BOTH: directed records, one count for a record's i, one for its k)
//   (rocprim::exclusive_scan of the packed counts, TopkPack: low word = an owner's segment start, high word = its output start)
//   topk_scatter_kernel  (key(J), partner) of every (directed) record into its owner's segment: 12 bytes each in two arrays
//   topk_select_kernel   one block per segment: MSB-first radix select of the K best, bitonic sort of the winners, records written
//   topk_threshold_kernel  a pass in row rounds: every owner's admission threshold for the next round
// Such a pass MERGES: the carried list C (directed records {owner, partner, V}, counted and scattered once, BOTH = false) and the round's
// new records (BOTH = true) go through the same count array, scan, segments and select.
// key(J): bits ^ 2^63 for a clear sign bit, ~bits for a set one -- a u64 whose unsigned order is the IEEE total order; its inverse is the
// same two cases told apart by the key's top bit, so the J bits come back exactly.
// The tile rule.  The i side arrives clustered by i (a query pass by query; an all-pairs pass bucketed by row where stage 2 groups, row
// by row from the dense kernel), and the two grouping kernels never issue one atomic per record on a hot owner's counter (a returning
// atomic on one address sustains ~87 operations/us chip-wide): a wave takes kTopkTile * 64 consecutive records
// and covers everything that carries the i of its first record with ONE atomic -- ballots give each step's mask of such lanes, the
// population counts add up to the run's length, and in the scatter a record's slot is the returned cursor plus the population count
// of the lanes below it; only the records behind a boundary inside a tile fall back to an atomic of their own.
// The k side of an all-pairs pass arrives in no order; it takes one atomic per record (no return value in the count kernel, a returned
// cursor in the scatter kernel).  Along a row the k are ascending, mostly consecutive, so a wave's 64 atomics fall on few cache
// lines; only a genome that is the larger member of very many pairs (a hub fed from the k side) makes one word hot.
#pragma once

namespace {

constexpr int kTopkMax = SELHIP_TOPK_MAX;       // largest K: the winners' sort area holds this many (key, rank) entries
constexpr int kTopkLdsCap = 4096;               // longest segment the select kernel stages in LDS ("query_topk_lds_cap")
constexpr int kTopkBlock = 512;                 // threads per segment: one compare-exchange per thread and step of the 1 024-entry sort
constexpr int kTopkTile = 8;                    // steps of 64 records a wave of the grouping kernels takes at a time
// LDS of topk_select_kernel: sort area (8 + 4 bytes per entry), staging area (the same per record), 256 bins, 4 control words --
// 61 KiB + 16 B: two blocks stay resident in a CU's 160 KiB
constexpr size_t kTopkLdsBytes = (size_t)(kTopkMax + kTopkLdsCap) * 12 + 256 * 4 + 16;
static_assert(2 * kTopkLdsBytes <= 160 * 1024, "two select blocks per CU");
static_assert(kTopkMax == 2 * kTopkBlock && (kTopkMax & (kTopkMax - 1)) == 0, "bitonic sort geometry");

__device__ __forceinline__ u64 topk_key(u64 bits) { return (bits >> 63) ? ~bits : bits ^ 0x8000000000000000ull; }
__device__ __forceinline__ u64 topk_unkey(u64 key) { return (key >> 63) ? key ^ 0x8000000000000000ull : ~key; }

// scan input: a query's record count c as (min(c, K) << 32) | c -- one scan yields the segment starts and the output starts
struct TopkPack {
    uint32_t k;
    __host__ __device__ u64 operator()(uint32_t c) const { return ((u64)(c < k ? c : k) << 32) | (u64)c; }
};

// cnt[n_own]: records per owner, zero on entry
template <bool BOTH>
__global__ __launch_bounds__(kBlock)
void topk_count_kernel(const selhip_pair_t* __restrict__ res, u64 n, int n_own, uint32_t* __restrict__ cnt) {
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
            const int k = BOTH && j < n ? res[j].k : -1;            // loaded with i, ahead of the atomics
            const bool same = i == i0;
            n0 += (uint32_t)__popcll(__ballot(same));
            if (!same && (unsigned)i < (unsigned)n_own) atomicAdd(&cnt[i], 1u);
            if constexpr (BOTH) {
                if ((unsigned)k < (unsigned)n_own) atomicAdd(&cnt[k], 1u);
            }
        }
        if (lane == 0 && (unsigned)i0 < (unsigned)n_own) atomicAdd(&cnt[i0], n0);
    }
}

// one slot of owner o's segment, drawn from its fill cursor
__device__ __forceinline__ u64 topk_slot(const u64* __restrict__ off, uint32_t* __restrict__ cur, int o) {
    return (u64)(uint32_t)off[o] + (u64)atomicAdd(&cur[o], 1u);
}

// the one clip: a position at or past seg_cap (a record without an owner in range, a cursor gone wrong) stores nothing
__device__ __forceinline__ void topk_put(u64* __restrict__ seg_key, uint32_t* __restrict__ seg_val, u64 seg_cap, u64 pos, u64 key, uint32_t val) {
    if (pos < seg_cap) { seg_key[pos] = key; seg_val[pos] = val; }
}

// cur[n_own]: fill cursors, zero on entry (one per owner: with BOTH, both sides draw from it).  off[o] low word = start of owner o's
// segment; seg_key / seg_val hold seg_cap entries (n, with BOTH 2 n), and seg_cap is also the position of a record that is not stored
template <bool BOTH>
__global__ __launch_bounds__(kBlock)
void topk_scatter_kernel(const selhip_pair_t* __restrict__ res, u64 n, int n_own, const u64* __restrict__ off, uint32_t* __restrict__ cur,
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
            rec[t] = j < n ? res4[j] : make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0, 0);        // past the end: no owner on either side
            same_mask[t] = __ballot((int)rec[t].x == i0);
            n0 += (uint32_t)__popcll(same_mask[t]);
        }
        const bool ok0 = (unsigned)i0 < (unsigned)n_own;
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
            } else if ((unsigned)i < (unsigned)n_own) {
                pos = topk_slot(off, cur, i);
            }
            at0 += (uint32_t)__popcll(same_mask[t]);
            topk_put(seg_key, seg_val, seg_cap, pos, key, (uint32_t)k);
            if constexpr (BOTH) {
                // owner k, partner i
                if ((unsigned)k < (unsigned)n_own) topk_put(seg_key, seg_val, seg_cap, topk_slot(off, cur, k), key, (uint32_t)i);
            }
        }
    }
}

// a ranks before b
__device__ __forceinline__ bool topk_before(u64 ka, uint32_t va, u64 kb, uint32_t vb) { return ka > kb || (ka == kb && va < vb); }

// The K best of L > K records into (skey, sval)[0, K), in no particular order.  The ranking is the descending order of the 96-bit
// composite (key, ~k); the select walks its 12 bytes from the top: a 256-bin histogram of the next byte over the records that match the
// bytes fixed so far, the bin that holds the K-th record found from the top, everything in the bins above it admitted, and the walk
// ends as soon as that bin holds exactly what is still needed -- at the latest with the last byte, since composites are unique.
// O(L) per pass; nothing is sorted.  keys / vals: the segment in LDS (staged) or in global memory (streamed every pass).
__device__ __forceinline__ void topk_radix_select(const u64* __restrict__ keys, const uint32_t* __restrict__ vals, uint32_t L, uint32_t K,
                                                  u64* skey, uint32_t* sval, uint32_t* hist, uint32_t* ctl) {
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const u64 lt = (1ull << lane) - 1ull;
    u64 pk = 0;                 // bytes fixed so far: of the key ...
    uint32_t pv = 0;            // ... and of ~k
    uint32_t need = K;
    int p = 0;
    for (;; ++p) {
        if (tid < 256) hist[tid] = 0;
        __syncthreads();
        for (uint32_t base = (uint32_t)wave * kWave; base < L; base += kTopkBlock) {
            const uint32_t t = base + lane;
            bool m = false;
            uint32_t d = 0;
            if (t < L) {
                const u64 key = keys[t];
                if (p < 8) {
                    m = p == 0 || (key >> (64 - 8 * p)) == (pk >> (64 - 8 * p));
                    d = (uint32_t)(key >> (56 - 8 * p)) & 255u;
                } else if (key == pk) {
                    const int s = p - 8;
                    const uint32_t nv = ~vals[t];
                    m = s == 0 || (nv >> (32 - 8 * s)) == (pv >> (32 - 8 * s));
                    d = (nv >> (24 - 8 * s)) & 255u;
                }
            }
            // the leading bytes of J are the same for most of a segment: the lanes that share the first lane's byte add once
            const u64 mm = __ballot(m);
            if (mm) {
                const int first = __ffsll((long long)mm) - 1;
                const uint32_t d0 = (uint32_t)__shfl((int)d, first, kWave);
                const bool same = m && d == d0;
                const u64 ms = __ballot(same);
                if (lane == first) atomicAdd(&hist[d0], (uint32_t)__popcll(ms));
                if (m && !same) atomicAdd(&hist[d], 1u);
            }
        }
        __syncthreads();
        if (wave == 0) {
            // lane l owns bins 255 - 4l .. 252 - 4l; inclusive scan of the lanes' sums from the top bin down
            uint32_t h[4], s = 0;
#pragma unroll
            for (int b = 0; b < 4; ++b) { h[b] = hist[255 - 4 * lane - b]; s += h[b]; }
            uint32_t inc = s;
#pragma unroll
            for (int w = 1; w < kWave; w <<= 1) { const uint32_t o = (uint32_t)__shfl_up((int)inc, w, kWave); if (lane >= w) inc += o; }
            uint32_t above = inc - s;
            if (above < need && inc >= need) {          // exactly one lane: the matching records are at least `need`
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    if (above + h[b] >= need) { ctl[0] = (uint32_t)(255 - 4 * lane - b); ctl[1] = above; ctl[2] = h[b]; break; }
                    above += h[b];
                }
            }
        }
        __syncthreads();
        const uint32_t bstar = ctl[0], hb = ctl[2];
        need -= ctl[1];
        if (p < 8) pk |= (u64)bstar << (56 - 8 * p);
        else       pv |= bstar << (24 - 8 * (p - 8));
        if (hb == need || p == 11) break;
    }
    // winners: the composite's first p + 1 bytes are at or above the threshold's
    if (tid == 0) ctl[3] = 0;
    __syncthreads();
    for (uint32_t base = (uint32_t)wave * kWave; base < L; base += kTopkBlock) {
        const uint32_t t = base + lane;
        bool win = false;
        u64 key = 0;
        if (t < L) {
            key = keys[t];
            if (p < 8) win = (key >> (56 - 8 * p)) >= (pk >> (56 - 8 * p));
            else       win = key > pk || (key == pk && ((~vals[t]) >> (24 - 8 * (p - 8))) >= (pv >> (24 - 8 * (p - 8))));
        }
        const u64 mw = __ballot(win);
        if (mw) {
            const int first = __ffsll((long long)mw) - 1;
            uint32_t at = 0;
            if (lane == first) at = atomicAdd(&ctl[3], (uint32_t)__popcll(mw));
            at = (uint32_t)__shfl((int)at, first, kWave) + (uint32_t)__popcll(mw & lt);
            if (win && at < (uint32_t)kTopkMax) { skey[at] = key; sval[at] = vals[t]; }
        }
    }
    __syncthreads();
}

// One block per query.  off[q] = (output start << 32) | segment start, off[q + 1] the next query's; segment length L:
//   L <= K        everything is a winner: straight into the sort area;
//   L <= LdsCap   the segment is staged in LDS once and the select's passes read it there;
//   longer        every pass of the select streams the keys from global memory.
// The <= K winners are then ordered by a bitonic sort in LDS and written as records at the output start.
__global__ __launch_bounds__(kTopkBlock)
void topk_select_kernel(const u64* __restrict__ seg_key, const uint32_t* __restrict__ seg_val, const u64* __restrict__ off, int K,
                        selhip_pair_t* __restrict__ out, u64 out_cap) {
    extern __shared__ __attribute__((aligned(16))) unsigned char topk_smem[];
    u64* skey = reinterpret_cast<u64*>(topk_smem);                              // [kTopkMax]
    u64* gkey = skey + kTopkMax;                                                // [kTopkLdsCap]
    uint32_t* sval = reinterpret_cast<uint32_t*>(gkey + kTopkLdsCap);           // [kTopkMax]
    uint32_t* gval = sval + kTopkMax;                                           // [kTopkLdsCap]
    uint32_t* hist = gval + kTopkLdsCap;                                        // [256]
    uint32_t* ctl = hist + 256;                                                 // [4]
    const int tid = threadIdx.x;
    const int q = (int)blockIdx.x;
    const u64 o0 = off[q], o1 = off[q + 1];
    const uint32_t s0 = (uint32_t)o0, L = (uint32_t)o1 - s0;
    if (L == 0) return;
    const u64 out0 = o0 >> 32;
    const uint32_t count = (uint32_t)((o1 >> 32) - out0);                       // min(L, K)
    const u64* __restrict__ kp = seg_key + s0;
    const uint32_t* __restrict__ vp = seg_val + s0;
    if (L <= (uint32_t)K) {
        for (uint32_t t = tid; t < L; t += kTopkBlock) { skey[t] = kp[t]; sval[t] = vp[t]; }
    } else if (L <= (uint32_t)kTopkLdsCap) {
        for (uint32_t t = tid; t < L; t += kTopkBlock) { gkey[t] = kp[t]; gval[t] = vp[t]; }
        __syncthreads();
        topk_radix_select(gkey, gval, L, (uint32_t)K, skey, sval, hist, ctl);
    } else {
        topk_radix_select(kp, vp, L, (uint32_t)K, skey, sval, hist, ctl);
    }
    // pad to a power of two with entries that rank last (key 0 is the image of no J that passes a threshold), then sort
    uint32_t n = 1;
    while (n < count) n <<= 1;
    for (uint32_t t = count + tid; t < n; t += kTopkBlock) { skey[t] = 0; sval[t] = 0xFFFFFFFFu; }
    __syncthreads();
    for (uint32_t k = 2; k <= n; k <<= 1) {
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            for (uint32_t t = tid; t < n; t += kTopkBlock) {
                const uint32_t x = t ^ j;
                if (x > t) {
                    const u64 ka = skey[t], kb = skey[x];
                    const uint32_t va = sval[t], vb = sval[x];
                    const bool up = (t & k) == 0;
                    if (up ? topk_before(kb, vb, ka, va) : topk_before(ka, va, kb, vb)) { skey[t] = kb; sval[t] = vb; skey[x] = ka; sval[x] = va; }
                }
            }
            __syncthreads();
        }
    }
    uint4* __restrict__ out4 = reinterpret_cast<uint4*>(out);
    for (uint32_t t = tid; t < count; t += kTopkBlock) {
        const u64 bits = topk_unkey(skey[t]);
        if (out0 + t < out_cap) out4[out0 + t] = make_uint4((uint32_t)q, sval[t], (uint32_t)bits, (uint32_t)(bits >> 32));
    }
}

// The admission thresholds of a top-k pass in row rounds (selhip_ctx_set_topk_rounds), behind the select of a round's merge: thr[g] =
// the value of owner g's K-th record in the reduced list `out` (its records stand at the output starts of `off`, in ranked order), and
// -inf for an owner that holds fewer than K.  off == nullptr: before the first round, -inf for every owner.
__global__ __launch_bounds__(kBlock)
void topk_threshold_kernel(const selhip_pair_t* __restrict__ out, u64 out_cap, const u64* __restrict__ off, int n_own, int K, double* __restrict__ thr) {
    const int g = (int)(blockIdx.x * kBlock + threadIdx.x);
    if (g >= n_own) return;
    double t = -__builtin_inf();
    if (off) {
        const u64 o0 = off[g] >> 32, o1 = off[g + 1] >> 32;
        if (o1 - o0 == (u64)K && o1 <= out_cap) t = out[o1 - 1].jaccard;
    }
    thr[g] = t;
}

}  // namespace

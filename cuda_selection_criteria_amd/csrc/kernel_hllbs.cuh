// kernel_hllbs.cuh -- stage 2a on BIT-SLICED HLL registers (p = 14): union histograms without LDS atomics.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace).
//
// What it computes is hll.h:1188-1204 (counts[max(a_r, b_r)]++ over the 16 384 registers of two sketches), bit for bit.
// How: the byte-per-register kernel (hll_union_hist_runs_kernel) issues one `ds_add_u32` per 64 registers and the LDS
// retires one of those every ~4.5 cycles per CU -- 1 150 cycles per pair per CU, whatever the memory system does.  Here a
// genome's registers are resident in HBM as SIX BIT PLANES (plane b = bit b of every register, 512 dwords each: 12 KiB per
// genome instead of 16, written once when the sketches are uploaded / attached), so that one 32-bit VALU operation
// handles 32 registers:
//   * max(a, b) bit-serially:  g = borrow chain of (b - a) from the LSB  (g = a > b),  M_b = g ? A_b : B_b      (3 ops per plane)
//   * the histogram of M by decoding its planes four values at a time: one v_bitop3_b32 picks the registers whose upper bits spell
//     the group, three more masks and four accumulating population counts (`v_bcnt_u32_b32`) give the group's four counts
//     (bs_group_node below).  Only the values below KHI (the pair's largest register value, rounded up to a multiple of 4) are decoded.
//   * the lanes' partial counts (<= 256 each) are packed two per dword and summed over the wave by a TRANSPOSING reduction
//     (v_permlane32_swap / v_permlane16_swap / DPP mirrors: each step halves the number of values a lane carries), 35 VALU
//     operations for all bins, after which lane L holds the totals of two bins and stores them.
// Per 32 x 64 registers: 2 NB + KHI boolean instructions (v_bitop3_b32, 2.2 cycles per SIMD: profiles/r03_bitplane_rate.txt) and KHI
// population counts (4.05 cycles), no LDS at all: ~1 500 cycles per pair per SIMD at KHI = 24, i.e. ~380 per CU.
#pragma once

namespace {

constexpr int kBsPlanes = 6;                                    // register values are < 64 (6 bits)
constexpr int kBsPlaneDwords = 512;                             // 16 384 registers / 32
constexpr int kBsGenomeDwords = kBsPlanes * kBsPlaneDwords;     // 12 KiB per genome
constexpr int kBsImagePlanes = 4;                               // the clamped image of a set with sparse lists (below): values 0..15
constexpr int kBsImageDwords = kBsImagePlanes * kBsPlaneDwords; // 8 KiB per genome, rows packed at that pitch
constexpr int kBsImageMaxT = 12;                                // thresholds up to which the image is exact

// hll_bitslice_kernel: one wave per genome.  Register r = 4 * ((8 o + jj) * 64 + lane) + s  (byte s of the dword the lane
// loads in step 8 o + jj) becomes bit 8 s + jj of dword o * 64 + lane of every plane: which bit a register lands on is
// irrelevant (a pair's counts are sums over all bits) as long as it is the same for every genome.
// gmax[g] = the largest register value of genome g, *max_val that of the set (values are taken modulo 64, like the byte kernel does).
__global__ __launch_bounds__(kBlock)
void hll_bitslice_kernel(const uint8_t* __restrict__ hll, long long n, uint32_t* __restrict__ bs, uint8_t* __restrict__ gmax,
                         int* __restrict__ max_val) {
    const int lane = threadIdx.x & (kWave - 1);
    uint32_t mx_all = 0;
    for (long long g = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; g < n; g += (long long)gridDim.x * kWavesPerBlock) {
        const uint32_t* row = reinterpret_cast<const uint32_t*>(hll + g * 16384);
        uint32_t* dst = bs + g * kBsGenomeDwords;
        uint32_t mx = 0;
#pragma unroll 1
        for (int o = 0; o < 8; ++o) {
            uint32_t d[8];
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) d[jj] = row[(o * 8 + jj) * kWave + lane] & 0x3F3F3F3Fu;
            uint32_t out[kBsPlanes];
#pragma unroll
            for (int b = 0; b < kBsPlanes; ++b) out[b] = 0;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const uint32_t w = d[jj];
                mx = max(max(mx, w & 0xFFu), max((w >> 8) & 0xFFu, max((w >> 16) & 0xFFu, w >> 24)));
#pragma unroll
                for (int b = 0; b < kBsPlanes; ++b) out[b] |= ((w >> b) & 0x01010101u) << jj;
            }
#pragma unroll
            for (int b = 0; b < kBsPlanes; ++b) dst[b * kBsPlaneDwords + o * kWave + lane] = out[b];
        }
#pragma unroll
        for (int s = 32; s > 0; s >>= 1) mx = max(mx, (uint32_t)__shfl_xor((int)mx, s, kWave));
        if (lane == 0) gmax[g] = (uint8_t)mx;
        mx_all = max(mx_all, mx);
    }
    if (lane == 0 && mx_all) atomicMax(max_val, (int)mx_all);
}

// ---- sparse lists of the rare high registers (stage 2a's "hist_sparse") --------------------------------------------------------
// A set's registers crowd the low values: at cfg3 a genome holds 58-68 of its 16 384 registers at 12 or more, and none above ~20.
// The bit-parallel decode costs the same for every group of four values however few registers it holds, so the groups from a
// threshold T up are taken out of it: every genome also keeps its registers >= T as a SORTED list of kBsSparseCap entries
// (r' << 8 | value, r' = 32 * plane dword + bit: the register's place in the planes; padded with kBsSparseNone), and stage 2a decodes
// only the values below T bit-parallel.  T = the smallest multiple of 4 at which every genome of the set holds at most
// kBsSparseCap such registers; above kBsSparseMaxT the set keeps the full decode.
constexpr int kBsSparseCap = 128;
constexpr int kBsSparseMaxT = 24;
constexpr uint32_t kBsSparseNone = 0xFFFFFFFFu;

// registers (one bit each) of a plane dword whose value is >= 4 k, from the planes 2..5 (a borrow chain of (v >> 2) - k; k wave-uniform)
__device__ __forceinline__ uint32_t bs_ge4k(const uint32_t (&p)[kBsPlanes], int k) {
    uint32_t borrow = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) borrow = ((k >> i) & 1) ? (~p[2 + i] | borrow) : (~p[2 + i] & borrow);
    return ~borrow;
}

// hll_sparse_t_kernel: one wave per genome; *t_need = max over the genomes of the smallest 4 k (1 <= k <= 6) with at most
// kBsSparseCap registers >= 4 k -- kBsSparseMaxT + 4 where even 24 leaves more.
__global__ __launch_bounds__(kBlock)
void hll_sparse_t_kernel(const uint32_t* __restrict__ bs, long long n, int* __restrict__ t_need) {
    const int lane = threadIdx.x & (kWave - 1);
    int t_all = 0;
    for (long long g = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; g < n; g += (long long)gridDim.x * kWavesPerBlock) {
        const uint32_t* src = bs + g * kBsGenomeDwords;
        int cnt[6] = {0, 0, 0, 0, 0, 0};
#pragma unroll 1
        for (int o = 0; o < kBsPlaneDwords / kWave; ++o) {
            uint32_t p[kBsPlanes];
#pragma unroll
            for (int b = 0; b < kBsPlanes; ++b) p[b] = src[b * kBsPlaneDwords + o * kWave + lane];
#pragma unroll
            for (int k = 1; k <= 6; ++k) cnt[k - 1] += __popc(bs_ge4k(p, k));
        }
        int t = kBsSparseMaxT + 4;
#pragma unroll
        for (int k = 6; k >= 1; --k) {
            int s = cnt[k - 1];
#pragma unroll
            for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, kWave);
            if (s <= kBsSparseCap) t = 4 * k;
        }
        t_all = max(t_all, t);
    }
    if (lane == 0 && t_all) atomicMax(t_need, t_all);
}

// hll_sparse_list_kernel: one wave per genome, its registers >= t (a multiple of 4 in [4, kBsSparseMaxT]) in ascending r', read from
// the planes 64 dwords at a time: each lane's count, a wave prefix sum for the offsets, the lane's entries in bit order.
// image (t <= kBsImageMaxT; else null): the genome's CLAMPED IMAGE, written from the same plane dwords -- the four planes of
// a' = min(a, 15), i.e. plane b < 4 = p[b] | p[4] | p[5], same bit placement, rows of kBsImageDwords.  max(a', b') = min(max(a, b), 15), so
// for T <= 12 the union's value is below T in the image exactly where it is in the full planes, and is then the same value: the
// decode of the groups below T reads four planes whatever the set's largest register is, and every value >= T comes from the lists.
// (Not for T >= 16: a 15 and a 16 would both read 15, and 15 is then below T.)
__global__ __launch_bounds__(kBlock)
void hll_sparse_list_kernel(const uint32_t* __restrict__ bs, long long n, int t, uint32_t* __restrict__ lists, uint32_t* __restrict__ image) {
    const int lane = threadIdx.x & (kWave - 1);
    for (long long g = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; g < n; g += (long long)gridDim.x * kWavesPerBlock) {
        const uint32_t* src = bs + g * kBsGenomeDwords;
        uint32_t* dst = lists + g * kBsSparseCap;
        int base = 0;
#pragma unroll 1
        for (int o = 0; o < kBsPlaneDwords / kWave; ++o) {
            const int d = o * kWave + lane;
            uint32_t p[kBsPlanes];
#pragma unroll
            for (int b = 0; b < kBsPlanes; ++b) p[b] = src[b * kBsPlaneDwords + d];
            if (image) {
                const uint32_t top = p[4] | p[5];
#pragma unroll
                for (int b = 0; b < kBsImagePlanes; ++b) image[g * kBsImageDwords + b * kBsPlaneDwords + d] = p[b] | top;
            }
            uint32_t h = bs_ge4k(p, t >> 2);
            const int cnt = __popc(h);
            int incl = cnt;
#pragma unroll
            for (int s = 1; s < kWave; s <<= 1) {
                const int v = __shfl_up(incl, s, kWave);
                if (lane >= s) incl += v;
            }
            int off = base + incl - cnt;
            while (h) {
                const int j = __builtin_ctz(h);
                h &= h - 1;
                uint32_t v = 0;
#pragma unroll
                for (int b = 0; b < kBsPlanes; ++b) v |= ((p[b] >> j) & 1u) << b;
                if (off < kBsSparseCap) dst[off] = ((uint32_t)(d * 32 + j) << 8) | v;
                ++off;
            }
            base += __shfl(incl, kWave - 1, kWave);
        }
        for (int i = lane; i < kBsSparseCap; i += kWave)
            if (i >= base) dst[i] = kBsSparseNone;
    }
}

// the lane's 8 dwords of each of the NB low planes of genome g (two 16-byte loads per plane, 1 KiB per wave instruction); PITCH = dwords
// from one genome's row to the next (kBsGenomeDwords: the six-plane rows, kBsImageDwords: the clamped image)
template <int NB, int PITCH = kBsGenomeDwords>
__device__ __forceinline__ void bs_load(const uint32_t* __restrict__ bs, int g, int lane, uint32_t (&r)[NB][8]) {
    static_assert(NB * kBsPlaneDwords <= PITCH, "a row holds the planes read");
    const uint4* p = reinterpret_cast<const uint4*>(bs + (size_t)g * PITCH);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const uint4 lo = p[b * (kBsPlaneDwords / 4) + lane], hi = p[b * (kBsPlaneDwords / 4) + kWave + lane];
        r[b][0] = lo.x; r[b][1] = lo.y; r[b][2] = lo.z; r[b][3] = lo.w;
        r[b][4] = hi.x; r[b][5] = hi.y; r[b][6] = hi.z; r[b][7] = hi.w;
    }
}

// ---- decoding the histogram of M = max(a, b) from its planes, four values at a time ----------------------------------------
// Group G = the values 4G .. 4G+3.  node = registers whose bits NB-1 .. 2 spell G: ONE v_bitop3_b32 from the planes (NB = 4: two
// inputs, NB = 5: three, NB = 6: a 2-input pre-node of bits 5, 4 and then three inputs).  Four population counts per group,
//   A = |node|,  B = |node & M1|,  C0 = |node & ~M1 & M0|,  C1 = |node & M1 & M0|     (each mask one more instruction)
// give  count(4G) = A - B - C0,  count(4G+1) = C0,  count(4G+2) = B - C1,  count(4G+3) = C1:  per decoded value one 2-cycle
// boolean instruction and one 4-cycle accumulating v_bcnt_u32_b32, and nothing for values nobody holds.
template <int TBL>
__device__ __forceinline__ uint32_t bs_op3(uint32_t a, uint32_t b, uint32_t c) { return __builtin_amdgcn_bitop3_b32(a, b, c, TBL); }
__device__ __forceinline__ void bs_count(uint32_t& acc, uint32_t mask) {
    // (the accumulating form spelled out: left to itself the compiler counts into fresh registers and sums them with v_add3_u32)
    asm("v_bcnt_u32_b32 %0, %1, %0" : "+v"(acc) : "v"(mask));
}

template <int NB, int G>
__device__ __forceinline__ uint32_t bs_group_node(const uint32_t (&M)[NB], const uint32_t (&pre)[4]) {
    constexpr int s1 = (G & 2) ? 0xCC : 0x33, s0 = (G & 1) ? 0xAA : 0x55;
    if constexpr (NB == 4)      return bs_op3<((G & 2) ? 0xF0 : 0x0F) & ((G & 1) ? 0xCC : 0x33)>(M[3], M[2], M[2]);
    else if constexpr (NB == 5) return bs_op3<((G & 4) ? 0xF0 : 0x0F) & s1 & s0>(M[4], M[3], M[2]);
    else                        return bs_op3<0xF0 & s1 & s0>(pre[G >> 2], M[3], M[2]);
}

// groups [G, GEND) of one column (compile-time recursion)
template <int NB, int G0, int G, int GEND>
__device__ __forceinline__ void bs_groups(const uint32_t (&M)[NB], const uint32_t (&pre)[4], uint32_t (&A)[GEND - G0], uint32_t (&B)[GEND - G0],
                                          uint32_t (&C0)[GEND - G0], uint32_t (&C1)[GEND - G0]) {
    if constexpr (G < GEND) {
        const uint32_t node = bs_group_node<NB, G>(M, pre);
        bs_count(A[G - G0], node);
        bs_count(B[G - G0], node & M[1]);
        bs_count(C0[G - G0], bs_op3<0xF0 & 0x33 & 0xAA>(node, M[1], M[0]));
        bs_count(C1[G - G0], bs_op3<0xF0 & 0xCC & 0xAA>(node, M[1], M[0]));
        bs_groups<NB, G0, G + 1, GEND>(M, pre, A, B, C0, C1);
    }
}

// the groups [G0, GE) of a pair (at most 6: 24 accumulators), all 8 columns; leaves the lane's packed partial counts in
// P[2 G0 .. 2 GE) (two values per dword).  A pair with more values takes another walk over the columns with the maximum recomputed
// (2 NB instructions per column) -- registers, not instructions, are what the kernel is short of.
template <int NB, int G0, int GE, int NP>
__device__ __forceinline__ void bs_decode(const uint32_t (&xa)[NB][8], const uint32_t (&yb)[NB][8], uint32_t (&P)[NP]) {
    constexpr int NG = GE - G0;
    static_assert(NG >= 1 && NG <= 6 && 2 * GE <= NP, "a chunk is 1..6 groups");
    uint32_t A[NG], B[NG], C0[NG], C1[NG];
#pragma unroll
    for (int v = 0; v < NG; ++v) { A[v] = 0; B[v] = 0; C0[v] = 0; C1[v] = 0; }
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        // g = a > b: the borrow of b - a, from the LSB: g' = (a & ~b) | (~(a ^ b) & g); then M = g ? a : b.  One v_bitop3_b32 each
        // (truth table = the expression on 0xF0, 0xCC, 0xAA; the compiler's own choice for the select is the 4-cycle v_bfi_b32)
        uint32_t g = 0;
#pragma unroll
        for (int b = 0; b < NB; ++b) g = bs_op3<0xB2>(xa[b][c], yb[b][c], g);
        uint32_t M[NB];
#pragma unroll
        for (int b = 0; b < NB; ++b) M[b] = bs_op3<0xCA>(g, xa[b][c], yb[b][c]);
        uint32_t pre[4] = {0u, 0u, 0u, 0u};
        if constexpr (NB == 6) {
            if constexpr (G0 < 4 && GE > 0)   pre[0] = bs_op3<0x0F & 0x33>(M[5], M[4], M[4]);
            if constexpr (G0 < 8 && GE > 4)   pre[1] = bs_op3<0x0F & 0xCC>(M[5], M[4], M[4]);
            if constexpr (G0 < 12 && GE > 8)  pre[2] = bs_op3<0xF0 & 0x33>(M[5], M[4], M[4]);
            if constexpr (G0 < 16 && GE > 12) pre[3] = bs_op3<0xF0 & 0xCC>(M[5], M[4], M[4]);
        }
        bs_groups<NB, G0, G0, GE>(M, pre, A, B, C0, C1);
    }
#pragma unroll
    for (int v = 0; v < NG; ++v) {
        P[2 * (G0 + v)]     = (A[v] - B[v] - C0[v]) | (C0[v] << 16);
        P[2 * (G0 + v) + 1] = (B[v] - C1[v]) | (C1[v] << 16);
    }
}

template <int CTRL>
__device__ __forceinline__ uint32_t bs_dpp(uint32_t v) {
    return (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, 0xF, 0xF, true);
}
constexpr int kDppRowMirror = 0x140, kDppRowHalfMirror = 0x141, kDppQuad3210 = 0x1B, kDppQuad1032 = 0xB1;

// Transposing wave reduction of 16 per-lane values: returns, in lane L, the sum over all 64 lanes of P[bs_pidx(L)].
// Each step exchanges half of the values a lane still carries for the partner's copies of the other half and adds:
//   v_permlane32_swap (lanes 32-63 of a <-> lanes 0-31 of b), v_permlane16_swap (odd rows of a <-> even rows of b),
//   then inside a row of 16 lanes: DPP row_mirror / row_half_mirror / quad_perm with a select per pair of values.
// NV: only P[0, NV) can be non-zero (the sparse kernel decodes 2 G1 packed values); the steps on values known to be zero are left out.
template <int NV = 16>
__device__ __forceinline__ uint32_t bs_reduce16(const uint32_t (&P)[16], int lane) {
    uint32_t Q[8], R[4];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        if (2 * j >= NV) { Q[j] = 0u; continue; }
        const auto s = __builtin_amdgcn_permlane32_swap(P[2 * j], P[2 * j + 1], false, false);
        Q[j] = s[0] + s[1];                 // lanes 0-31: P[2j] over {i, i+32}; lanes 32-63: P[2j+1]
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        if (4 * j >= NV) { R[j] = 0u; continue; }
        const auto s = __builtin_amdgcn_permlane16_swap(Q[2 * j], Q[2 * j + 1], false, false);
        R[j] = s[0] + s[1];                 // rows 0..3: P[4j], P[4j+2], P[4j+1], P[4j+3], each over 4 source lanes per lane
    }
    const bool h = (lane & 8) != 0, q = (lane & 4) != 0;
    const uint32_t t0 = R[0] + bs_dpp<kDppRowMirror>(R[0]);
    const uint32_t t1 = NV > 4 ? R[1] + bs_dpp<kDppRowMirror>(R[1]) : 0u;
    const uint32_t t2 = NV > 8 ? R[2] + bs_dpp<kDppRowMirror>(R[2]) : 0u;
    const uint32_t t3 = NV > 12 ? R[3] + bs_dpp<kDppRowMirror>(R[3]) : 0u;
    const uint32_t S0 = h ? t1 : t0, S1 = h ? t3 : t2;
    const uint32_t u0 = S0 + bs_dpp<kDppRowHalfMirror>(S0);
    const uint32_t u1 = NV > 8 ? S1 + bs_dpp<kDppRowHalfMirror>(S1) : 0u;
    const uint32_t U = q ? u1 : u0;
    const uint32_t V = U + bs_dpp<kDppQuad3210>(U);
    return V + bs_dpp<kDppQuad1032>(V);
}
__device__ __forceinline__ int bs_pidx(int lane) {
    const int r = lane >> 4;
    return 4 * (2 * ((lane >> 2) & 1) + ((lane >> 3) & 1)) + (((r & 1) << 1) | (r >> 1));
}

// union histogram of one pair from the two rows' planes: returns, in lane L, the packed totals of the bins 2 * pidx(L), 2 * pidx(L) + 1
// (lanes 0, 1 of a quad) or 32 + ... (lanes 2, 3).  kp (wave-uniform) = values the pair can hold: every register of both rows is < kp.
// The first 24 values (16 with four planes) are always decoded; the walks for 24.., 32.., 48.. only when the pair can hold such values
// -- a typical sketch's largest register is ~log2(cardinality) - 11 while a set of 10 000 reaches 30.  (One code path with optional
// walks, not a body per size: with several bodies in one kernel the compiler hoists their common maximum computation above the
// branch and keeps it live -- 84 VGPRs for one body, 166 for two.)
template <int NB>
__device__ __forceinline__ uint32_t bs_pair_hist(const uint32_t (&xa)[NB][8], const uint32_t (&yb)[NB][8], int kp, int lane) {
    constexpr int NP = NB == 6 ? 32 : 16;                                 // packed values: two bins per dword (a wave total is <= 16 384)
    uint32_t P[NP];
#pragma unroll
    for (int v = 0; v < NP; ++v) P[v] = 0u;
    if constexpr (NB == 4) {
        bs_decode<NB, 0, 4, NP>(xa, yb, P);
    } else {
        bs_decode<NB, 0, 6, NP>(xa, yb, P);
        if (kp > 24) bs_decode<NB, 6, 8, NP>(xa, yb, P);
        if constexpr (NB == 6) {
            if (kp > 32) bs_decode<NB, 8, 12, NP>(xa, yb, P);
            if (kp > 48) bs_decode<NB, 12, 16, NP>(xa, yb, P);
        }
    }
    // the transposing reduction, 16 packed values at a time
    uint32_t lo[16];
#pragma unroll
    for (int v = 0; v < 16; ++v) lo[v] = P[v];
    uint32_t tot = bs_reduce16(lo, lane);
    if constexpr (NP > 16) {
        uint32_t tot_hi = 0;
        if (kp > 32) {
#pragma unroll
            for (int v = 0; v < 16; ++v) lo[v] = P[16 + v];
            tot_hi = bs_reduce16(lo, lane);
        }
        tot = (lane & 2) ? tot_hi : tot;
    } else {
        tot = (lane & 2) ? 0u : tot;
    }
    return tot;
}

// ---- the values >= T of a pair from the two rows' sparse lists (A = query row x, B = candidate row y) ---------------------------
// A register r with M_r = max(a_r, b_r) >= T is in A or in B.  The query row's histogram of A (hA: lane L keeps the bin it stores)
// counts every r of A at a_r; each entry of B then corrects it: r not in A adds b_r; r in A with b_r > a_r moves one count from a_r to
// b_r; r in A with b_r <= a_r changes nothing.  Membership and a_r come from a wave-private LDS image of A, built once per query row:
// a bitmap of its r' (512 dwords), the rank of the first entry of every dword that holds one, and the values by rank -- an entry's
// rank is first[w] + |bits[w] below it|.  Exact (no hashing, so no collisions), two dependent LDS reads per entry of B.
struct alignas(16) BsSparseLds {
    uint32_t bits[kBsPlaneDwords];      // A's registers, one bit each at r'
    uint32_t bins[64];                  // the pair's corrections by value (zero between pairs; the lane storing bin v reads and clears it)
    uint8_t first[kBsPlaneDwords];      // rank of the first entry of A in each dword of bits that holds one
    uint8_t val[kBsSparseCap];          // A's values by rank
};

// the query row x's image in sp and its histogram hA (the bin my_bin); every lane of the wave takes part
__device__ __forceinline__ uint32_t bs_sparse_row(BsSparseLds* sp, const uint32_t* __restrict__ lists, int x, int lane, int my_bin) {
    const uint32_t e0 = lists[(size_t)x * kBsSparseCap + lane], e1 = lists[(size_t)x * kBsSparseCap + kWave + lane];
    uint4* bits4 = reinterpret_cast<uint4*>(sp->bits);
    bits4[2 * lane] = make_uint4(0u, 0u, 0u, 0u);
    bits4[2 * lane + 1] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t e = h ? e1 : e0;
        if (e != kBsSparseNone) {
            const uint32_t r = e >> 8;
            atomicOr(&sp->bits[r >> 5], 1u << (r & 31));
            atomicAdd(&sp->bins[e & 63], 1u);
            sp->val[h * kWave + lane] = (uint8_t)(e & 63);
        }
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const uint32_t e = h ? e1 : e0;
        if (e != kBsSparseNone) {
            const uint32_t r = e >> 8;
            // every entry of a dword writes the same rank
            sp->first[r >> 5] = (uint8_t)(h * kWave + lane - __popc(sp->bits[r >> 5] & ((1u << (r & 31)) - 1u)));
        }
    }
    const uint32_t hA = sp->bins[my_bin];
    sp->bins[my_bin] = 0u;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    return hA;
}

// one entry of B against the image of A
__device__ __forceinline__ void bs_sparse_entry(BsSparseLds* sp, uint32_t e) {
    if (e == kBsSparseNone) return;
    const uint32_t r = e >> 8, v = e & 63, w = sp->bits[r >> 5], below = w & ((1u << (r & 31)) - 1u);
    if ((w >> (r & 31)) & 1u) {
        const uint32_t av = sp->val[sp->first[r >> 5] + __popc(below)];
        if (v > av) {
            atomicAdd(&sp->bins[v], 1u);
            atomicSub(&sp->bins[av], 1u);
        }
    } else {
        atomicAdd(&sp->bins[v], 1u);
    }
}

// hll_union_hist_bs_kernel<NB, G1>: same contract as hll_union_hist_runs_kernel (window [chunk_off, chunk_off + chunk_len) of the
// pair list, counts indexed from the window start, tasks of run_len (at most 64) consecutive pairs, block b works in the (b % 8)-th eighth of
// the tasks = on XCD b % 8), on the bit planes.  NB = planes that can be non-zero in the SET (4, 5 or 6).
// G1 = 0: how many values are decoded is decided PER PAIR from the two rows' largest register values (gmax, written with the planes).
// G1 > 0 (the set's sparse threshold T = 4 G1, `lists` its sparse lists): the groups [0, G1) are decoded bit-parallel, in one walk,
// and every value >= T comes from the lists (bs_sparse_row / bs_sparse_entry); gmax is not read.
// PITCH = dwords per row of `bs`: kBsGenomeDwords, or kBsImageDwords where `bs` is the set's clamped image (NB = 4, G1 <= 3, whatever the
// set's largest register: hll_sparse_list_kernel).
// One wave per pair: a lane owns 8 dwords (256 registers) of every plane; the query row's planes stay in registers across a run.
template <int NB, int G1, int PITCH = kBsGenomeDwords>
__global__ __launch_bounds__(kBlock, NB <= 5 ? 4 : 2)
void hll_union_hist_bs_kernel(const uint32_t* __restrict__ bs, const uint8_t* __restrict__ gmax, const uint32_t* __restrict__ lists,
                              const selhip_int2_t* __restrict__ pairs, const u64* __restrict__ n_pairs_dev, u64 cap, uint32_t* __restrict__ counts,
                              u64 chunk_off, u64 chunk_len, int run_len, u64 dense_pairs) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = threadIdx.x / kWave;
    u64 n_pairs = *n_pairs_dev;
    if (n_pairs > cap) n_pairs = cap;
    n_pairs = n_pairs > chunk_off ? min(n_pairs - chunk_off, chunk_len) : 0;
    pairs += chunk_off;
    // A SHORT list runs on part of the grid: the device holds 1 024 SIMDs x (4 or 2) waves of this kernel at a time, and a wave's first
    // pair costs three dependent round trips (count, pair record, rows) before any arithmetic.  With 8 192 waves for 16 000 pairs (one of
    // 8 ranks of the weak-scaled workload) every wave took two pairs and half of the waves could only start when the first half had
    // ended: 44 us for 16 us of arithmetic.  Up to eight pairs per resident wave the list is therefore dealt to at most ONE round of
    // waves (the other blocks leave at once); longer lists keep the whole grid, whose two rounds of shorter waves end more evenly.
    u64 blocks_active = gridDim.x;
    {
        const u64 resident = 1024ull * (NB <= 5 ? 4 : 2);
        if (n_pairs <= 8 * resident) {
            const u64 waves = min(resident, max(n_pairs, (u64)64));
            blocks_active = min((u64)gridDim.x, ((waves + 8 * kWavesPerBlock - 1) / (8 * kWavesPerBlock)) * 8);
        }
    }
    if (blockIdx.x >= blocks_active) return;
    const u64 stride = (blocks_active >> 3) * kWavesPerBlock;             // waves per XCD (the host launches a multiple of 8 blocks)
    const int my_bin = ((lane & 2) ? 32 : 0) + 2 * bs_pidx(lane) + (lane & 1);
    // A DENSE survivor graph (n_pairs >= dense_pairs; the host sets 32 pairs per query row of the pass on a grouped list, "hist_dense_degree"): a query
    // row has tens to hundreds of partners spread over the whole table, the table does not fit one L2 (4 MiB = ~400 rows) and in list
    // order every pair fetches its candidate row from beyond it (the 25 %-degenerate set of bench.py: 730 000 pairs among 2 516 genomes,
    // 6.2 GB per pass at 92 % of the Infinity Cache's gather rate).  Then every XCD walks the WHOLE list, 64 pairs per task, and takes
    // the pairs whose candidate row hashes to it: its L2 only ever sees an eighth of the candidate rows (they stay) plus the query rows,
    // which all its waves pass through together (the list is query-major).  Same counts in the same slots either way.
    const bool dense = n_pairs >= dense_pairs;
    const uint32_t xcd = blockIdx.x & 7u;
    // Runs only pay (the query row stays in registers) once every wave has several of them: on the whole grid a list is dealt out in
    // runs of n_pairs / 16 per wave at most (one of 8 ranks of cfg4, 56 000 pairs on 8 192 waves: 49.9 us with single pairs, 58.3 us with
    // runs of 4).  A short list on its one round of waves gives every wave ONE run of its n_pairs / waves consecutive pairs: with single
    // pairs every pair fetched both of its rows (one of 8 ranks at 28 280 genomes: 16 000 pairs, 41 us for 16 us of arithmetic).
    const u64 waves_active = 8 * stride;
    // (runs of at most 2 there: longer ones put the uses of a candidate row at different points of different waves' serial chains
    //  and it leaves L2 in between -- one chunk lane of a rank of cfg4, 28 000 pairs, table 512 MB: 47.3 / 49.2 / 56.3 us with runs of
    //  1 / 2 / 4; the 16 000-pair share above: 40.1 / 37.1 / 37.3)
    const bool short_list = blocks_active < gridDim.x;
    const u64 per_wave = short_list ? (n_pairs + waves_active - 1) / waves_active : n_pairs / (16 * stride);
    run_len = dense ? kWave : (int)max((u64)1, min((u64)min(run_len, short_list ? 2 : kWave), per_wave));
    const u64 n_tasks = (n_pairs + run_len - 1) / run_len;
    const u64 tasks_per_xcd = dense ? n_tasks : (n_tasks + 7) >> 3;
    const u64 t_begin = dense ? 0 : (u64)xcd * tasks_per_xcd, t_end = min(t_begin + tasks_per_xcd, n_tasks);
    int cur_x = -1;
    uint32_t xa[NB][8];
    BsSparseLds* sp = nullptr;
    uint32_t hA = 0;                                                      // G1 > 0: the query row's count of bin my_bin over its list
    if constexpr (G1 > 0) {
        __shared__ BsSparseLds sp_block[kWavesPerBlock];
        sp = &sp_block[wave];
        sp->bins[my_bin] = 0u;
    }
    for (u64 task = t_begin + (u64)(blockIdx.x >> 3) * kWavesPerBlock + wave; task < t_end; task += stride) {
        const u64 j0 = task * run_len;
        const int cnt = (int)min((u64)run_len, n_pairs - j0);
        selhip_int2_t pr{0, 0};
        if (lane < cnt) pr = pairs[j0 + lane];                            // the task's pairs, one per lane
        u64 mine = __ballot(lane < cnt && (!dense || (((uint32_t)pr.y * 0x9E3779B1u) >> 29) == xcd));
        while (mine) {
            const int src = (int)__builtin_ctzll(mine);
            mine &= mine - 1;
            const int px = __builtin_amdgcn_readlane(pr.x, src), py = __builtin_amdgcn_readlane(pr.y, src);   // wave-uniform: scalar row addresses
            uint32_t yb[NB][8];
            bs_load<NB, PITCH>(bs, py, lane, yb);
            if constexpr (G1 == 0) {
                if (px != cur_x) { bs_load<NB, PITCH>(bs, px, lane, xa); cur_x = px; }
                const int kp = max((int)gmax[px], (int)gmax[py]) + 1;     // values this pair can hold: [0, kp)
                const uint32_t tot = bs_pair_hist<NB>(xa, yb, kp, lane);
                counts[(j0 + src) * 64 + my_bin] = (lane & 1) ? (tot >> 16) : (tot & 0xFFFFu);
            } else {
                const uint32_t eb0 = lists[(size_t)py * kBsSparseCap + lane], eb1 = lists[(size_t)py * kBsSparseCap + kWave + lane];
                if (px != cur_x) { bs_load<NB, PITCH>(bs, px, lane, xa); hA = bs_sparse_row(sp, lists, px, lane, my_bin); cur_x = px; }
                uint32_t P[16];
#pragma unroll
                for (int v = 0; v < 16; ++v) P[v] = 0u;
                bs_decode<NB, 0, G1, 16>(xa, yb, P);
                const uint32_t tot = bs_reduce16<2 * G1>(P, lane);
                bs_sparse_entry(sp, eb0);
                bs_sparse_entry(sp, eb1);
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const uint32_t s = sp->bins[my_bin];
                sp->bins[my_bin] = 0u;
                // (bins >= 32 hold nothing dense: the lanes with lane & 2 store the sparse counts alone)
                const uint32_t dense_cnt = (lane & 2) ? 0u : ((lane & 1) ? (tot >> 16) : (tot & 0xFFFFu));
                counts[(j0 + src) * 64 + my_bin] = dense_cnt + hA + s;
            }
        }
    }
}

// (Round 3 also built this kernel with the NEXT pair's candidate planes prefetched through LDS -- every wave a slot of NB x 2 KiB filled by
// LDS-DMA (`global_load_lds_dwordx4`) while the current pair is decoded, pair records and maxima read two pairs ahead; bit-identical in
// the parity suite.  It changed nothing: cfg3 53.7 -> 56.6 us, hard 0.874 -> 0.878 ms, cfg4 / cfg5 equal (gpurun_out/r03/g_pf*).  The PMC
// pass says why (profiles/r03b_pmc_summary.json): the vector units are ACTIVE for 0.71 of the kernel at cfg3 and 0.83 on the hard set --
// ~4.1 cycles per instruction: in this mix of dependent chains the boolean instructions do not reach the 2.2 cycles they show alone --
// so the waves are not waiting for memory, they are waiting for each other's arithmetic.  Dropped.)
//
// What bounds the sparse form <NB, 3> (profiles/hist_image_ab.txt, cfg3: 45 000 pairs, T = 12).  Not vector issue alone: 17.5 M
// wave-instructions (SQ_INSTS_VALU; 389 a pair) on 1 024 SIMDs in 37.8 us is ~5 cycles per instruction, the units ~60 % busy.  Not bytes
// through the CU alone either: the clamped image takes a fifth of the plane bytes away -- the L2 read requests fall to 0.79 (5.33 M ->
// 4.19 M, TCP_TCC_READ_REQ_sum), 16 boolean instructions and 16 VGPRs per pair go with the fifth plane (118 -> 102 VGPRs, still 4 waves
// per SIMD; 5 would spill) -- and the kernel goes from 37.8 to 34.4 us, 9 %, where the bytes fell by 19 %.  The same set clamped at 15 on
// the six-plane rows had predicted 39.5 -> 36.7 us.  The dense walk of the 25 %-degenerate set, 730 000 pairs whose candidate rows come
// from one L2, gains the same share (533 -> 489 us), and beyond the Infinity Cache the shorter rows turn the lists from a loss into a
// gain (host_pass.hpp, sparse_t_used).  So each pair is a chain -- pair record, rows, decode, list entries through LDS, store -- of which
// the row fetch is one link among several, with four waves per SIMD to hide it; the run length makes no difference (1 / 2 / 4 / 8
// within the spread).  Sharing a candidate row among the waves of a block through LDS would take most of the remaining row traffic
// out of L2; not built.

}  // namespace

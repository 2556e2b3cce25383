// kernel_fold.cuh -- hll_fold_kernel: the auxiliary HLL sketches [n][1 << p_aux] folded from the main registers [n][1 << p]
// (selhip_hll_fold, selhip_ctx_fold_aux_hll, selhip_ctx_fold_queries_aux_hll).  The rule is hll_fold.hpp; this file only walks memory.
// Part of libselhip.so; included by selection_kernels.hip only.
//
// A row is 2^p bytes and a group -- the registers of one output register -- 2^d aligned bytes of it, d = p - p_aux, so the n rows
// fold as ONE flat array of (n << p) / 16 sixteen-byte vectors, whatever the row length (p = 4: a row is one vector).  Every input
// byte is read once, 16 B per lane, the lanes of a wave 1 KiB in a row, kFoldLoads loads per lane in flight; 2^-d as many bytes
// are written.  The group width meets that load shape in three ways (FoldShape):
//   kFoldInLane        d = 0 .. 4    a lane's vector holds 16 >> d whole groups: no lane talks to another, a lane stores 16 >> d bytes
//   kFoldAcrossLanes   d = 5 .. 10   a group is the vectors of 2^(d - 4) neighbouring lanes of one wave-wide load: every lane folds its
//                                    vector, a butterfly of d - 4 __shfl_xor steps combines them, the group's first lane stores a byte
//   kFoldAcrossLoads   d = 11 .. 16  (p >= 15) a group is 2^(d - 10) wave-wide loads: one wave per group, a running combine per lane
//                                    over its loads, one wave-wide butterfly at the end, lane 0 stores a byte
// Inside a vector the walk uses the shortcut hll_fold.hpp states: offsets ascend with the address, so a run's combine is the
// contribution of its first non-empty byte -- found with a count of trailing zeros, not with a byte loop (a streaming kernel on this
// chip has some 80 vector operations per lane and vector to spend before arithmetic, not HBM, bounds it; a byte loop takes them all).
#pragma once

namespace {

constexpr int kFoldLoads = 4;          // 16-byte loads per lane in flight: 8 waves per CU then hold the 32 KiB a CU needs to stream
constexpr unsigned kFoldMaxBlocks = 1u << 18;

enum FoldShape { kFoldInLane = 0, kFoldAcrossLanes = 1, kFoldAcrossLoads = 2 };

// contribution of a run of up to 8 consecutive registers (byte j of v = the register at dropped bits t0 + j, little endian)
template <class T>
__device__ __forceinline__ unsigned fold_run(T v, unsigned t0, unsigned d) {
    const unsigned b = v ? (unsigned)(sizeof(T) == 8 ? __builtin_ctzll((u64)v) : __builtin_ctz((unsigned)v)) >> 3 : 0u;
    const unsigned r = (unsigned)(v >> (b * 8)) & 0xFFu;          // (0 when the whole run is empty)
    return selhip::fold_contrib(r, t0 + b, d);
}

// the same for a lane's whole vector: 16 registers from dropped bits t0
__device__ __forceinline__ unsigned fold_run16(const uint4& w, unsigned t0, unsigned d) {
    const u64 x = (u64)w.x | ((u64)w.y << 32), y = (u64)w.z | ((u64)w.w << 32);
    return x ? fold_run(x, t0, d) : fold_run(y, t0 + 8u, d);
}

// kFoldInLane: the 16 >> D output bytes of one vector, stored with one instruction
template <int D>
__device__ __forceinline__ void fold_store_in_lane(const uint4& w, uint8_t* __restrict__ out, u64 vec) {
    if constexpr (D == 0) {
        reinterpret_cast<uint4*>(out)[vec] = w;
    } else if constexpr (D <= 2) {
        constexpr int W = 1 << D, kPerDword = 4 >> D;                                  // bytes per group, groups per dword
        constexpr unsigned kMask = D == 1 ? 0xFFFFu : 0xFFFFFFFFu;
        const unsigned dw[4] = {w.x, w.y, w.z, w.w};
        unsigned o[4 * kPerDword];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int g = 0; g < kPerDword; ++g) o[q * kPerDword + g] = fold_run<unsigned>((dw[q] >> (g * 8 * W)) & kMask, 0u, D);
        if constexpr (D == 1) {
            uint2 v;
            v.x = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
            v.y = o[4] | (o[5] << 8) | (o[6] << 16) | (o[7] << 24);
            reinterpret_cast<uint2*>(out)[vec] = v;
        } else {
            reinterpret_cast<uint32_t*>(out)[vec] = o[0] | (o[1] << 8) | (o[2] << 16) | (o[3] << 24);
        }
    } else if constexpr (D == 3) {
        const u64 x = (u64)w.x | ((u64)w.y << 32), y = (u64)w.z | ((u64)w.w << 32);
        reinterpret_cast<uint16_t*>(out)[vec] = (uint16_t)(fold_run(x, 0u, 3u) | (fold_run(y, 0u, 3u) << 8));
    } else {
        out[vec] = (uint8_t)fold_run16(w, 0u, 4u);
    }
}

// in = the rows as n_vec 16-byte vectors, out = (n_vec * 16) >> d bytes.  D is the template's d for kFoldInLane and kFoldAcrossLanes;
// kFoldAcrossLoads takes d from the argument (D = 0).  Blocks of kBlock threads; any grid (the loops stride by it).
template <int SHAPE, int D>
__global__ __launch_bounds__(kBlock) void hll_fold_kernel(const uint4* __restrict__ in, uint8_t* __restrict__ out, u64 n_vec, int d_arg) {
    if constexpr (SHAPE == kFoldAcrossLoads) {
        // one wave per group of 2^(d - 10) wave-wide loads
        const unsigned d = (unsigned)d_arg;
        const int lane = threadIdx.x & (kWave - 1);
        const u64 loads = (u64)1 << (d - 10), n_groups = (n_vec * 16) >> d;
        const u64 n_waves = (u64)gridDim.x * kWavesPerBlock;
        for (u64 g = (u64)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; g < n_groups; g += n_waves) {
            const uint4* src = in + g * loads * kWave;
            unsigned acc = 0;
            for (u64 l0 = 0; l0 < loads; l0 += kFoldLoads) {
                uint4 w[kFoldLoads];
#pragma unroll
                for (int k = 0; k < kFoldLoads; ++k) w[k] = l0 + k < loads ? src[(l0 + k) * kWave + lane] : make_uint4(0, 0, 0, 0);
#pragma unroll
                for (int k = 0; k < kFoldLoads; ++k)
                    acc = selhip::fold_combine(acc, fold_run16(w[k], (unsigned)(((l0 + k) * kWave + lane) * 16), d));
            }
            for (int s = kWave / 2; s > 0; s >>= 1) acc = selhip::fold_combine(acc, (unsigned)__shfl_xor((int)acc, s, kWave));
            if (lane == 0) out[g] = (uint8_t)acc;
        }
    } else {
        constexpr u64 kPerBlock = (u64)kBlock * kFoldLoads;
        const u64 stride = (u64)gridDim.x * kPerBlock;
        for (u64 base = (u64)blockIdx.x * kPerBlock; base < n_vec; base += stride) {       // (block-uniform: the shuffles below see whole waves)
            uint4 w[kFoldLoads];
#pragma unroll
            for (int k = 0; k < kFoldLoads; ++k) {
                const u64 vec = base + (u64)k * kBlock + threadIdx.x;
                w[k] = vec < n_vec ? in[vec] : make_uint4(0, 0, 0, 0);
            }
#pragma unroll
            for (int k = 0; k < kFoldLoads; ++k) {
                const u64 vec = base + (u64)k * kBlock + threadIdx.x;
                if constexpr (SHAPE == kFoldInLane) {
                    if (vec < n_vec) fold_store_in_lane<D>(w[k], out, vec);
                } else {
                    // a wave's 64 vectors start at a multiple of 64 and n_vec is a multiple of the group's L: a group is whole or absent
                    constexpr unsigned L = 1u << (D - 4);
                    const unsigned sub = threadIdx.x & (L - 1u);
                    unsigned c = fold_run16(w[k], sub * 16u, (unsigned)D);
#pragma unroll
                    for (unsigned s = 1; s < L; s <<= 1) c = selhip::fold_combine(c, (unsigned)__shfl_xor((int)c, (int)s, kWave));
                    if (sub == 0 && vec < n_vec) out[vec >> (D - 4)] = (uint8_t)c;
                }
            }
        }
    }
}

template <int SHAPE, int D>
hipError_t launch_hll_fold_as(hipStream_t s, unsigned grid, const uint8_t* in, uint8_t* out, u64 n_vec, int d) {
    hipLaunchKernelGGL((hll_fold_kernel<SHAPE, D>), dim3(grid), dim3(kBlock), 0, s, reinterpret_cast<const uint4*>(in), out, n_vec, d);
    return hipGetLastError();
}

// in [n][1 << p] -> out [n][1 << p_aux], both 16-byte aligned; 4 <= p_aux <= p <= 20, p - p_aux <= 16, n > 0 (the callers checked)
hipError_t launch_hll_fold(hipStream_t s, const uint8_t* in, u64 n, int p, int p_aux, uint8_t* out) {
    const int d = p - p_aux;
    const u64 n_vec = (n << p) >> 4;
    const u64 vec_blocks = (n_vec + (u64)kBlock * kFoldLoads - 1) / ((u64)kBlock * kFoldLoads);
    const unsigned grid = (unsigned)std::min<u64>(vec_blocks, kFoldMaxBlocks);
    switch (d) {
        case 0: return launch_hll_fold_as<kFoldInLane, 0>(s, grid, in, out, n_vec, d);
        case 1: return launch_hll_fold_as<kFoldInLane, 1>(s, grid, in, out, n_vec, d);
        case 2: return launch_hll_fold_as<kFoldInLane, 2>(s, grid, in, out, n_vec, d);
        case 3: return launch_hll_fold_as<kFoldInLane, 3>(s, grid, in, out, n_vec, d);
        case 4: return launch_hll_fold_as<kFoldInLane, 4>(s, grid, in, out, n_vec, d);
        case 5: return launch_hll_fold_as<kFoldAcrossLanes, 5>(s, grid, in, out, n_vec, d);
        case 6: return launch_hll_fold_as<kFoldAcrossLanes, 6>(s, grid, in, out, n_vec, d);
        case 7: return launch_hll_fold_as<kFoldAcrossLanes, 7>(s, grid, in, out, n_vec, d);
        case 8: return launch_hll_fold_as<kFoldAcrossLanes, 8>(s, grid, in, out, n_vec, d);
        case 9: return launch_hll_fold_as<kFoldAcrossLanes, 9>(s, grid, in, out, n_vec, d);
        case 10: return launch_hll_fold_as<kFoldAcrossLanes, 10>(s, grid, in, out, n_vec, d);
        default: {
            const u64 n_groups = n << p_aux;                                       // one wave each
            const u64 blocks = (n_groups + kWavesPerBlock - 1) / kWavesPerBlock;
            return launch_hll_fold_as<kFoldAcrossLoads, 0>(s, (unsigned)std::min<u64>(blocks, kFoldMaxBlocks), in, out, n_vec, d);
        }
    }
}

}  // namespace

// kernel_gather.cuh -- the winner-takes-all screen (include/selection_hip.h section 2m; selhip_ctx_gather / selhip_gather): every query's
// bucket row decomposed greedily into database rows.  Exact integer work in two stages.
// Part of libselhip.so; included by selection_kernels.hip only (one translation unit, anonymous namespace), behind kernel_matrix_smh.cuh
// (the unit of the fast path, matrix_smh_q) and host_plan.hpp (matrix_units).
//   MASK STAGE -- which database rows share at least c_min buckets with a query, and WHICH buckets: a candidate entry is
//   {database rank, |M(d)|} plus the W = ceil(m / 32) words of M(d).  The rows are streamed twice, count then fill, with two scan launches
//   between: the segments are sized exactly, nothing is appended through an atomic, and a segment comes out in rank order (which no
//   output depends on: the pick compares (count, rank) explicitly).
//     gather_mask_kernel<NCH, FILL>   m = 128 NCH: matrix_smh_kernel's enumeration (Q query rows per wave in VGPRs, the span's <= 64
//       candidate rows streamed past them through the same ring).  The 2 NCH v_cmp_eq_u64 ballots of a pair stay in their SGPR pairs; a
//       pair whose raw count reaches c_min ANDs them with the query's `bucket filled` ballots (formed only then), counts again, and a
//       survivor's ballots are its mask -- lane l < 2 NCH selects ballot l and stores it with one 8-byte vector store.  The lane map of
//       the coalesced loads permutes the bits: ballot 2 c + h, bit l = bucket 128 c + 2 l + h.  Every candidate of a query, and the
//       query's own valid mask (gather_valid_kernel), use that one map.  FILL = false tallies the survivors per (query, span).
//     gather_mask_narrow_kernel<G, FILL>   m = 128 / G, G in {2, 4}: matrix_smh_narrow_kernel's enumeration (Q = 12 query rows per wave,
//       one u64x2 each, replicated over the G lane groups; a wave load = G consecutive candidate rows through the same ring).  The two
//       ballots of a (row, load) hold G fields of 64 / G bits; matrix_smh_narrow_counts splits the raw counts, and a (row, group) that
//       reaches c_min ANDs its fields with the query row's `bucket filled` fields and counts again.  A survivor's fields are its mask.
//     gather_mask_wide_kernel<FILL>   m = 1 024 C, C in {2, 3, 4}: two phases per (wave, span).  Phase 1 is matrix_smh_wide_kernel's walk
//       (Q = 3 rows, chunk-major, ring of two): lane l ends with the RAW count of column k0 + l.  Phase 2 takes the columns whose raw
//       count reaches c_min in ascending order on the scalar unit and walks the C chunks of that one pair again (both rows in L2 by
//       then): 16 ballots per chunk, ANDed with the query chunk's `bucket filled` ballots, the masked count added up, and the ballots
//       PARKED -- lane l < 16 keeps ballot l of chunk c in one u64 register -- because only the last chunk decides.  A survivor's parked
//       words are stored, C 8-byte stores per lane; nothing is stored for a pair that fails (its slot belongs to the next cell).
//     gather_mask_generic_kernel<FILL>   every other m <= 4 096, rows that are not 16-byte aligned, and every non-tile m under
//       "gather_generic": one query row per wave, lane = column of the span.
//     THE BIT MAPS of a mask (one per kernel; a query's valid mask, gather_valid_*_kernel, and all of its candidates' masks share it, and
//     no output depends on which):
//       tile     u64 word 2 c + h, bit l = bucket 128 c + 2 l + h                              (c < NCH, h = 0 for .x, 1 for .y)
//       wide     u64 word 16 c' + 2 c + h, bit l = bucket 1 024 c' + 128 c + 2 l + h           (the tile map of NCH = 8 per chunk c' < C)
//       narrow   m = 64: dword h, bit l = bucket 2 l + h;  m = 32: ONE dword, bit l = bucket 2 l, bit 16 + l = bucket 2 l + 1 (l < 16)
//       generic  natural order: dword w, bit b = bucket 32 w + b; padding bits zero
//     gather_scan_rows_kernel / gather_scan_queries_kernel   the tallies of a query's spans into exclusive offsets in place and a total,
//       the totals into 64-bit segment starts, the number of candidates and the longest segment.
//   PICK STAGE -- gather_pick_kernel<WT>: one workgroup per query, all rounds in one launch.  A segment that fits the LDS the launch was
//   given is staged once, word-major ([word][candidate], then the ranks: a wave's lanes read consecutive dwords); a longer one is read
//   from global memory every round.  A round: lane t takes the candidates t, t + 256, ..., popcount(mask & live) over the words -- live
//   wave-uniform, in scalar registers for W <= WT in {4, 8, 16, 32}, in LDS for WT = 0 --, keeps its best (count, smaller rank) as one
//   64-bit key, the wave reduces by butterfly, the four waves through LDS (one barrier; the slots alternate), every wave clears the
//   winner's words from its copy of live and thread 0 stores the pick.  No spin, no wait on another workgroup.
#pragma once

namespace {

constexpr int kGatherMaxM = 4096;
constexpr int kGatherMaxW = kGatherMaxM / 32;
constexpr u64 kGatherEmpty = ~0ull;                   // an unfilled bucket

struct GatherCand { int rank, count; };                 // count = |M(d)|, the pick's `matches`

constexpr int gather_words(int m) { return (m + 31) / 32; }

// `n` wave-uniform 64-bit values, one per lane l < N, to dst[l] (8-byte aligned): a select chain and ONE vector store per lane
template <int N>
__device__ __forceinline__ void gather_store_ballots(u64* __restrict__ dst, const u64 (&b)[N], int lane) {
    u64 v = 0;
#pragma unroll
    for (int i = 0; i < N; ++i) v = lane == i ? b[i] : v;
    if (lane < N) dst[lane] = v;
}

// valid[q][W]: the query's filled buckets under the map its candidates' masks use (FAST: the fast path's lane map; else natural order)
template <int NCH>
__global__ __launch_bounds__(kBlock)
void gather_valid_kernel(const u64* __restrict__ X, int m, int n_q, uint32_t* __restrict__ valid) {
    const int lane = threadIdx.x & (kWave - 1);
    const int W = gather_words(m);
    for (long long i = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < n_q; i += (long long)gridDim.x * kWavesPerBlock) {
        if constexpr (NCH > 0) {
            const u64x2* row = reinterpret_cast<const u64x2*>(X) + i * (NCH * kWave) + lane;
            u64 b[2 * NCH];
#pragma unroll
            for (int c = 0; c < NCH; ++c) {
                const u64x2 v = row[c * kWave];
                b[2 * c] = __ballot(v.x != kGatherEmpty);
                b[2 * c + 1] = __ballot(v.y != kGatherEmpty);
            }
            gather_store_ballots<2 * NCH>(reinterpret_cast<u64*>(valid + i * W), b, lane);
        } else {
            const u64* x = X + i * m;
            for (int w = lane; w < W; w += kWave) {
                uint32_t word = 0;
                for (int b = 0; b < 32 && 32 * w + b < m; ++b) word |= (x[32 * w + b] != kGatherEmpty ? 1u : 0u) << b;
                valid[i * W + w] = word;
            }
        }
    }
}

// the narrow form: a wave load is G query rows, lane group g holds row i + g; lane g < G stores the fields of its row
template <int G>
__global__ __launch_bounds__(kBlock)
void gather_valid_narrow_kernel(const u64x2* __restrict__ X, int n_q, uint32_t* __restrict__ valid) {
    constexpr int LPR = kWave / G;
    const int lane = threadIdx.x & (kWave - 1);
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    for (long long i = ((long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave) * G; i < n_q; i += (long long)gridDim.x * kWavesPerBlock * G) {
        const u64x2 v = X[min(i + grp, (long long)n_q - 1) * LPR + sub];      // groups past the set re-read the last row, never stored
        const u64 bx = __ballot(v.x != kGatherEmpty), by = __ballot(v.y != kGatherEmpty);
        if (lane < G && i + lane < n_q) {
            if constexpr (G == 2) reinterpret_cast<u64*>(valid)[i + lane] = (u64)(uint32_t)(bx >> (32 * lane)) | ((by >> (32 * lane)) << 32);
            else valid[i + lane] = ((uint32_t)(bx >> (16 * lane)) & 0xFFFFu) | ((uint32_t)(by >> (16 * lane)) << 16);
        }
    }
}

// the wide form: n_chunks chunks of the NCH = 8 map
__global__ __launch_bounds__(kBlock)
void gather_valid_wide_kernel(const u64x2* __restrict__ X, int n_chunks, int n_q, uint32_t* __restrict__ valid) {
    constexpr int NCH = kMatrixSmhWideNch;
    const int lane = threadIdx.x & (kWave - 1);
    for (long long i = (long long)blockIdx.x * kWavesPerBlock + threadIdx.x / kWave; i < n_q; i += (long long)gridDim.x * kWavesPerBlock) {
        for (int c = 0; c < n_chunks; ++c) {
            const u64x2* row = X + (i * n_chunks + c) * (NCH * kWave) + lane;
            u64 b[2 * NCH];
#pragma unroll
            for (int h = 0; h < NCH; ++h) {
                const u64x2 v = row[h * kWave];
                b[2 * h] = __ballot(v.x != kGatherEmpty);
                b[2 * h + 1] = __ballot(v.y != kGatherEmpty);
            }
            gather_store_ballots<2 * NCH>(reinterpret_cast<u64*>(valid + (i * n_chunks + c) * (4 * NCH)), b, lane);
        }
    }
}

// the mask stage of the fast path.  span_cnt[n_q][n_spans]: FILL = false writes every cell's survivor count; FILL = true reads the
// exclusive offsets the row scan left there and, with qstart[q], stores survivor s of a cell at qstart[q] + offset + s
template <int NCH, bool FILL>
__global__ __launch_bounds__(kBlock, (NCH <= 4 ? 3 : 2))
void gather_mask_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_q, int n_y, int n_tiles, long long n_units, int c_min,
                        long long n_spans, uint32_t* __restrict__ span_cnt, const u64* __restrict__ qstart, GatherCand* __restrict__ cand,
                        uint32_t* __restrict__ masks) {
    constexpr int Q = matrix_smh_q(NCH);
    constexpr int ROWV = NCH * kWave;
    constexpr int AHEAD = NCH <= 4 ? kStreamAhead : 1;
    constexpr int RING = AHEAD + 1;
    constexpr int NB = 2 * NCH;                        // ballots per pair = u64 words of a mask
    static_assert(Q <= kWave, "one lane per query row holds its segment position");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long span = 8 * (j / n_tiles) + (u & 7);
        const long long k0l = span * kMatrixSpan;
        if (k0l >= n_y) continue;
        const long long i0l = ((j % n_tiles) * kWavesPerBlock + wave) * Q;
        if (i0l >= n_q) continue;                                            // wave-uniform; the kernel has no block barrier
        const int i0 = (int)i0l, k0 = (int)k0l;
        const int ke = (int)min((long long)n_y, k0l + kMatrixSpan);
        u64x2 q[Q][NCH];
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            const u64x2* row = X + (long long)min(i0 + a, n_q - 1) * ROWV + lane;     // rows past the set: a valid row, never stored
#pragma unroll
            for (int c = 0; c < NCH; ++c) q[a][c] = row[c * kWave];
        }
        int ns[Q];                                                           // survivors of (row a, this span) so far; wave-uniform
#pragma unroll
        for (int a = 0; a < Q; ++a) ns[a] = 0;
        u64 vbase = 0;                                                       // FILL: lane a = where row a's survivors of this span start
        if (FILL && lane < Q && i0 + lane < n_q) vbase = qstart[i0 + lane] + span_cnt[(long long)(i0 + lane) * n_spans + span];
        u64x2 ring[RING][NCH];
        auto load_row = [&](u64x2 (&dst)[NCH], int kk) {
            const u64x2* row = Y + (long long)min(kk, ke - 1) * ROWV + lane;         // clamped: prefetches past the span re-read a valid row
#pragma unroll
            for (int c = 0; c < NCH; ++c) dst[c] = row[c * kWave];
        };
        auto compare_row = [&](const u64x2 (&cd)[NCH], int kk) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                u64 b[NB];
                int cnt = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    b[2 * c] = __ballot(cd[c].x == q[a][c].x);
                    b[2 * c + 1] = __ballot(cd[c].y == q[a][c].y);
                    cnt += __popcll(b[2 * c]) + __popcll(b[2 * c + 1]);
                }
                if (cnt < c_min) continue;                                   // (the raw count bounds the masked one from above)
                cnt = 0;
#pragma unroll
                for (int c = 0; c < NCH; ++c) {
                    b[2 * c] &= __ballot(q[a][c].x != kGatherEmpty);
                    b[2 * c + 1] &= __ballot(q[a][c].y != kGatherEmpty);
                    cnt += __popcll(b[2 * c]) + __popcll(b[2 * c + 1]);
                }
                if (cnt < c_min || i0 + a >= n_q) continue;
                if constexpr (FILL) {
                    const u64 base = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(vbase >> 32), a) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)vbase, a);
                    const u64 slot = base + (u64)ns[a];
                    if (lane == 0) cand[slot] = GatherCand{kk, cnt};
                    gather_store_ballots<NB>(reinterpret_cast<u64*>(masks + slot * (u64)(2 * NB)), b, lane);
                }
                ns[a] += 1;
            }
        };
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) load_row(ring[s], k0 + s);
        for (int k = k0; k < ke; k += RING) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                const int kk = k + s;
                if (kk >= ke) break;
                load_row(ring[(s + AHEAD) % RING], kk + AHEAD);
                compare_row(ring[s], kk);
            }
        }
        if constexpr (!FILL) {
            int mine = 0;
#pragma unroll
            for (int a = 0; a < Q; ++a) mine = lane == a ? ns[a] : mine;
            if (lane < Q && i0 + lane < n_q) span_cnt[(long long)(i0 + lane) * n_spans + span] = (uint32_t)mine;
        }
    }
}

// ---- narrow rows: m = 32 and m = 64 -----------------------------------------------------------------------------------------------
// the mask stage of m = 128 / G: the tile kernel's survivor counting over matrix_smh_narrow_kernel's loads.  A cell's survivors come in
// ascending rank in both launches: the loads ascend, and within a load g ascends
template <int G, bool FILL>
__global__ __launch_bounds__(kBlock, 3)
void gather_mask_narrow_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_q, int n_y, int n_tiles, long long n_units, int c_min,
                               long long n_spans, uint32_t* __restrict__ span_cnt, const u64* __restrict__ qstart, GatherCand* __restrict__ cand,
                               uint32_t* __restrict__ masks) {
    constexpr int Q = kMatrixSmhNarrowQ;
    constexpr int LPR = kWave / G;                     // u64x2 (lanes) per sketch row = bits of a ballot field: m = 2 LPR
    constexpr int AHEAD = kStreamAhead;
    constexpr int RING = AHEAD + 1;
    static_assert(kMatrixSpan % G == 0, "a span is whole wave loads");
    static_assert(Q <= kWave, "one lane per query row holds its segment position");
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int sub = lane & (LPR - 1), grp = lane / LPR;
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long span = 8 * (j / n_tiles) + (u & 7);
        const long long k0l = span * kMatrixSpan;
        if (k0l >= n_y) continue;
        const long long i0l = ((j % n_tiles) * kWavesPerBlock + wave) * Q;
        if (i0l >= n_q) continue;                                            // wave-uniform; the kernel has no block barrier
        const int i0 = (int)i0l, k0 = (int)k0l;
        const int ke = (int)min((long long)n_y, k0l + kMatrixSpan);
        u64x2 q[Q];
#pragma unroll
        for (int a = 0; a < Q; ++a) q[a] = X[(long long)min(i0 + a, n_q - 1) * LPR + sub];     // every lane group holds the whole row; rows past the set: a valid row, never stored
        // lane a = survivors of (row a, this span) so far.  Wave-uniform per row, but kept in ONE VGPR and touched only when a pair
        // survives: twelve scalar counters on top of the ballots were more than the SGPR file holds
        int ns = 0;
        u64 vbase = 0;                                                       // FILL: lane a = where row a's survivors of this span start
        if (FILL && lane < Q && i0 + lane < n_q) vbase = qstart[i0 + lane] + span_cnt[(long long)(i0 + lane) * n_spans + span];
        u64x2 ring[RING];
        auto load_rows = [&](u64x2& dst, int kk) { dst = Y[(long long)min(kk + grp, ke - 1) * LPR + sub]; };     // a group past the span re-reads row ke - 1
        auto compare_rows = [&](const u64x2& cd, int kk) {
#pragma unroll
            for (int a = 0; a < Q; ++a) {
                const u64 bx = __ballot(cd.x == q[a].x), by = __ballot(cd.y == q[a].y);      // (the two ballots matrix_smh_narrow_counts forms: one pair of compares)
                int raw[G];
                matrix_smh_narrow_counts<G>(q[a], cd, raw);
                bool any = false;
#pragma unroll
                for (int g = 0; g < G; ++g) any = any || (raw[g] >= c_min && kk + g < ke);
                if (!any || i0 + a >= n_q) continue;                         // (the raw count bounds the masked one from above)
                // the query row's `bucket filled` fields, formed only now: field 0 of each ballot (every group holds the row)
                // (behind an empty asm on the constant, so that the compiler does not hoist the 2 Q loop-invariant ballots into SGPRs it lacks)
                u64 empty = kGatherEmpty;
                asm volatile("" : "+s"(empty));
                const uint32_t vx = (uint32_t)__ballot(q[a].x != empty), vy = (uint32_t)__ballot(q[a].y != empty);
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    if (raw[g] < c_min || kk + g >= ke) continue;
                    uint32_t w0, w1 = 0;
                    if constexpr (G == 2) {
                        w0 = (uint32_t)(bx >> (LPR * g)) & vx;
                        w1 = (uint32_t)(by >> (LPR * g)) & vy;
                    } else {
                        w0 = (((uint32_t)(bx >> (LPR * g)) & 0xFFFFu) | ((uint32_t)(by >> (LPR * g)) << 16)) & ((vx & 0xFFFFu) | (vy << 16));
                    }
                    const int cnt = __popc(w0) + __popc(w1);
                    if (cnt < c_min) continue;
                    if constexpr (FILL) {
                        const u64 base = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(vbase >> 32), a) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)vbase, a);
                        const u64 slot = base + (u64)(uint32_t)__builtin_amdgcn_readlane(ns, a);
                        if (lane == 0) {
                            cand[slot] = GatherCand{kk + g, cnt};
                            if constexpr (G == 2) *reinterpret_cast<u64*>(masks + slot * 2) = (u64)w0 | ((u64)w1 << 32);
                            else masks[slot] = w0;
                        }
                    }
                    ns = matrix_smh_writelane(__builtin_amdgcn_readlane(ns, a) + 1, a, ns);
                }
            }
        };
#pragma unroll
        for (int s = 0; s < AHEAD; ++s) load_rows(ring[s], k0 + s * G);
        for (int k = k0; k < ke; k += RING * G) {
#pragma unroll
            for (int s = 0; s < RING; ++s) {
                const int kk = k + s * G;
                if (kk >= ke) break;
                load_rows(ring[(s + AHEAD) % RING], kk + AHEAD * G);
                compare_rows(ring[s], kk);
            }
        }
        if constexpr (!FILL) {
            if (lane < Q && i0 + lane < n_q) span_cnt[(long long)(i0 + lane) * n_spans + span] = (uint32_t)ns;
        }
    }
}

// ---- wide rows: m = 1024 C, C = 2 .. 4 ------------------------------------------------------------------------------------------------
template <bool FILL>
__global__ __launch_bounds__(kBlock, 2)
void gather_mask_wide_kernel(const u64x2* __restrict__ X, const u64x2* __restrict__ Y, int n_chunks, int n_q, int n_y, int n_tiles, long long n_units, int c_min,
                             long long n_spans, uint32_t* __restrict__ span_cnt, const u64* __restrict__ qstart, GatherCand* __restrict__ cand,
                             uint32_t* __restrict__ masks) {
    constexpr int NCH = kMatrixSmhWideNch;
    constexpr int Q = matrix_smh_q(NCH);
    constexpr int CHV = NCH * kWave;                   // u64x2 per chunk of a row
    constexpr int NB = 2 * NCH;                        // ballots per (pair, chunk) = u64 words of a chunk's mask
    constexpr int MAXC = kGatherMaxM / (2 * CHV);      // the parking registers: one u64 per chunk
    const long long pitch = (long long)n_chunks * CHV; // u64x2 per sketch row
    const u64 W = (u64)(2 * NB) * (u64)n_chunks;       // dwords of a mask
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long span = 8 * (j / n_tiles) + (u & 7);
        const long long k0l = span * kMatrixSpan;
        if (k0l >= n_y) continue;
        const long long i0l = ((j % n_tiles) * kWavesPerBlock + wave) * Q;
        if (i0l >= n_q) continue;                                            // wave-uniform; the kernel has no block barrier
        const int i0 = (int)i0l, k0 = (int)k0l;
        const int ke = (int)min((long long)n_y, k0l + kMatrixSpan);
        int acc[Q];                                                          // lane l: the running RAW count of column k0 + l
#pragma unroll
        for (int a = 0; a < Q; ++a) acc[a] = 0;
        {
            // phase 1, matrix_smh_wide_kernel's walk: ONE stream of (chunk, candidate row) steps, chunk-major, through a ring of two
            u64x2 q[Q][NCH];
            auto load_queries = [&](int c) {
#pragma unroll
                for (int a = 0; a < Q; ++a) {
                    const u64x2* row = X + (long long)min(i0 + a, n_q - 1) * pitch + (long long)c * CHV + lane;      // rows past the set: a valid row, never stored
#pragma unroll
                    for (int h = 0; h < NCH; ++h) q[a][h] = row[h * kWave];
                }
            };
            u64x2 ring[2][NCH];
            int pc = 0, pk = k0;                                             // the step to fetch next (wave-uniform)
            auto prefetch = [&](u64x2 (&dst)[NCH]) {
                const u64x2* row = Y + (long long)pk * pitch + (long long)pc * CHV + lane;
#pragma unroll
                for (int h = 0; h < NCH; ++h) dst[h] = row[h * kWave];
                if (pk + 1 < ke) ++pk;
                else if (pc + 1 < n_chunks) { pk = k0; ++pc; }               // (behind the last step: that step again)
            };
            int cc = 0, ck = k0;                                             // the step to compare next
            auto compare_row = [&](const u64x2 (&cd)[NCH]) {
                const int col = ck - k0;
#pragma unroll
                for (int a = 0; a < Q; ++a) {
                    const int cnt = matrix_smh_chunk_count<NCH>(q[a], cd) + __builtin_amdgcn_readlane(acc[a], col);
                    acc[a] = matrix_smh_writelane(cnt, col, acc[a]);
                }
                if (++ck == ke) {
                    ck = k0;
                    if (++cc < n_chunks) load_queries(cc);
                }
            };
            const int steps = n_chunks * (ke - k0);
            prefetch(ring[0]);
            load_queries(0);
            for (int t = 0; t < steps; t += 2) {
                prefetch(ring[1]);
                compare_row(ring[0]);
                if (t + 1 >= steps) break;
                prefetch(ring[0]);
                compare_row(ring[1]);
            }
        }
        // phase 2: the pairs whose raw count reaches c_min, one at a time in ascending rank; the phase-1 registers are dead
        int ns[Q];                                                           // survivors of (row a, this span) so far; wave-uniform
#pragma unroll
        for (int a = 0; a < Q; ++a) ns[a] = 0;
        u64 vbase = 0;                                                       // FILL: lane a = where row a's survivors of this span start
        if (FILL && lane < Q && i0 + lane < n_q) vbase = qstart[i0 + lane] + span_cnt[(long long)(i0 + lane) * n_spans + span];
#pragma unroll
        for (int a = 0; a < Q; ++a) {
            u64 todo = __ballot(acc[a] >= c_min && k0 + lane < ke);
            if (i0 + a >= n_q) todo = 0;
            const u64x2* const qrow = X + (long long)min(i0 + a, n_q - 1) * pitch + lane;
            while (todo) {
                const int col = __builtin_ctzll(todo);
                todo &= todo - 1;
                const u64x2* const crow = Y + (long long)(k0 + col) * pitch + lane;
                u64 park[MAXC];
                int cnt = 0;
#pragma unroll
                for (int c = 0; c < MAXC; ++c) {
                    park[c] = 0;
                    if (c >= n_chunks) continue;
                    u64x2 qc[NCH], cd[NCH];
#pragma unroll
                    for (int h = 0; h < NCH; ++h) { qc[h] = qrow[c * CHV + h * kWave]; cd[h] = crow[c * CHV + h * kWave]; }
                    u64 v = 0;
#pragma unroll
                    for (int h = 0; h < NCH; ++h) {
                        const u64 bx = __ballot(cd[h].x == qc[h].x) & __ballot(qc[h].x != kGatherEmpty);
                        const u64 by = __ballot(cd[h].y == qc[h].y) & __ballot(qc[h].y != kGatherEmpty);
                        cnt += __popcll(bx) + __popcll(by);
                        v = lane == 2 * h ? bx : lane == 2 * h + 1 ? by : v;  // (the select chain of gather_store_ballots)
                    }
                    park[c] = v;
                }
                if (cnt < c_min) continue;
                if constexpr (FILL) {
                    const u64 base = ((u64)(uint32_t)__builtin_amdgcn_readlane((int)(vbase >> 32), a) << 32) | (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)vbase, a);
                    const u64 slot = base + (u64)ns[a];
                    if (lane == 0) cand[slot] = GatherCand{k0 + col, cnt};
                    if (lane < NB) {
                        u64* const dst = reinterpret_cast<u64*>(masks + slot * W) + lane;
#pragma unroll
                        for (int c = 0; c < MAXC; ++c)
                            if (c < n_chunks) dst[c * NB] = park[c];
                    }
                }
                ns[a] += 1;
            }
        }
        if constexpr (!FILL) {
            int mine = 0;
#pragma unroll
            for (int a = 0; a < Q; ++a) mine = lane == a ? ns[a] : mine;
            if (lane < Q && i0 + lane < n_q) span_cnt[(long long)(i0 + lane) * n_spans + span] = (uint32_t)mine;
        }
    }
}

// the mask stage for every other m: matrix_smh_generic_kernel's unit, masks in natural bucket order
template <bool FILL>
__global__ __launch_bounds__(kBlock)
void gather_mask_generic_kernel(const u64* __restrict__ X, const u64* __restrict__ Y, int m, int n_q, int n_y, int n_tiles, long long n_units, int c_min,
                                long long n_spans, uint32_t* __restrict__ span_cnt, const u64* __restrict__ qstart, GatherCand* __restrict__ cand,
                                uint32_t* __restrict__ masks) {
    const int lane = threadIdx.x & (kWave - 1);
    const int wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x / kWave);
    const int W = gather_words(m);
    for (long long u = blockIdx.x; u < n_units; u += gridDim.x) {
        const long long j = u >> 3;
        const long long span = 8 * (j / n_tiles) + (u & 7);
        const long long k0 = span * kMatrixSpan;
        if (k0 >= n_y) continue;
        const long long row = (j % n_tiles) * kWavesPerBlock + wave;
        if (row >= n_q) continue;
        const int ky = (int)k0 + lane;
        const u64* const x = X + row * m;
        const u64* const y = Y + (long long)min(ky, n_y - 1) * m;            // lanes past the end: a valid row, never stored
        int cnt = 0;
        for (int b = 0; b < m; ++b) cnt += (x[b] == y[b] && x[b] != kGatherEmpty) ? 1 : 0;
        const bool ok = ky < n_y && cnt >= c_min;
        const u64 okb = __ballot(ok);
        const long long cell = row * n_spans + span;
        if constexpr (!FILL) {
            if (lane == 0) span_cnt[cell] = (uint32_t)__popcll(okb);
        } else if (ok) {
            const u64 slot = qstart[row] + span_cnt[cell] + (u64)__popcll(okb & ((1ull << lane) - 1ull));
            cand[slot] = GatherCand{ky, cnt};
            for (int w = 0; w < W; ++w) {
                uint32_t word = 0;
                for (int b = 0; b < 32 && 32 * w + b < m; ++b) {
                    const u64 xv = x[32 * w + b];
                    word |= (xv == y[32 * w + b] && xv != kGatherEmpty ? 1u : 0u) << b;
                }
                masks[slot * (u64)W + w] = word;
            }
        }
    }
}

// exclusive prefix of v over the block's kBlock threads and the block's sum; two barriers; lds: kWavesPerBlock slots
__device__ __forceinline__ u64 gather_block_exscan(u64 v, u64* lds, u64* total) {
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    u64 inc = v;
#pragma unroll
    for (int s = 1; s < kWave; s <<= 1) {
        const u64 o = __shfl_up(inc, s);
        if (lane >= s) inc += o;
    }
    if (lane == kWave - 1) lds[wave] = inc;
    __syncthreads();
    u64 before = 0, tot = 0;
#pragma unroll
    for (int w = 0; w < kWavesPerBlock; ++w) {
        const u64 x = lds[w];
        before += w < wave ? x : 0;
        tot += x;
    }
    __syncthreads();
    *total = tot;
    return before + inc - v;
}

// one workgroup per query: span_cnt[q][0 .. n_spans) to exclusive offsets in place, qtot[q] = their sum
__global__ __launch_bounds__(kBlock)
void gather_scan_rows_kernel(uint32_t* __restrict__ span_cnt, long long n_spans, int n_q, uint32_t* __restrict__ qtot) {
    __shared__ u64 lds[kWavesPerBlock];
    for (long long q = blockIdx.x; q < n_q; q += gridDim.x) {
        uint32_t* const row = span_cnt + q * n_spans;
        u64 carry = 0;
        for (long long base = 0; base < n_spans; base += kBlock) {
            const long long s = base + threadIdx.x;
            const uint32_t v = s < n_spans ? row[s] : 0u;
            u64 tot;
            const u64 ex = gather_block_exscan(v, lds, &tot);
            if (s < n_spans) row[s] = (uint32_t)(carry + ex);
            carry += tot;
        }
        if (threadIdx.x == 0) qtot[q] = (uint32_t)carry;                     // (at most n_D < 2^31 survivors per query)
    }
}

// ONE workgroup: qstart[q] = the candidates of the queries before q, qstart[n_q] = all of them, qstart[n_q + 1] = the longest segment
__global__ __launch_bounds__(kBlock)
void gather_scan_queries_kernel(const uint32_t* __restrict__ qtot, int n_q, u64* __restrict__ qstart) {
    __shared__ u64 lds[kWavesPerBlock];
    __shared__ uint32_t longest;
    if (threadIdx.x == 0) longest = 0;
    __syncthreads();
    u64 carry = 0;
    uint32_t mine = 0;
    for (long long base = 0; base < n_q; base += kBlock) {
        const long long q = base + threadIdx.x;
        const uint32_t v = q < n_q ? qtot[q] : 0u;
        mine = max(mine, v);
        u64 tot;
        const u64 ex = gather_block_exscan(v, lds, &tot);
        if (q < n_q) qstart[q] = carry + ex;
        carry += tot;
    }
    atomicMax(&longest, mine);
    __syncthreads();
    if (threadIdx.x == 0) { qstart[n_q] = carry; qstart[n_q + 1] = longest; }
}

// no database row: every segment empty (n + 2 words of zero; a kernel, so that the call can be captured)
__global__ __launch_bounds__(kBlock)
void gather_clear_kernel(u64* __restrict__ p, long long n) {
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) p[i] = 0;
}

struct GatherOut {
    selhip_gather_pick_t* picks;      // [n_q][max_picks]
    int* n_picks;                     // [n_q]
    int* unexplained;                 // [n_q]   each may be null
};

// the pick stage.  lds_words: the dwords of dynamic LDS the launch was given for staging; stage[] = [W][n_c] mask words, then [n_c] ranks
template <int WT>
__global__ __launch_bounds__(kBlock)
void gather_pick_kernel(int W, int c_min, int max_picks, long long lds_words, const u64* __restrict__ qstart, const GatherCand* __restrict__ cand,
                        const uint32_t* __restrict__ masks, const uint32_t* __restrict__ valid, GatherOut o) {
    extern __shared__ uint32_t stage[];
    __shared__ u64 wkey[2][kWavesPerBlock];
    __shared__ int widx[2][kWavesPerBlock];
    __shared__ uint32_t live_l[WT == 0 ? kGatherMaxW : 1];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const long long q = blockIdx.x;
    const u64 start = qstart[q];
    const int n_c = (int)(qstart[q + 1] - start);
    const bool staged = (long long)n_c * (W + 1) <= lds_words;               // workgroup-uniform
    const GatherCand* const cq = cand + start;
    const uint32_t* const mq = masks + start * (u64)W;
    if (staged) {
        for (int i = tid; i < n_c; i += kBlock) {
            for (int w = 0; w < W; ++w) stage[w * n_c + i] = mq[(u64)i * W + w];
            stage[W * n_c + i] = (uint32_t)cq[i].rank;
        }
    }
    uint32_t live[WT == 0 ? 1 : WT];
    if constexpr (WT > 0) {
#pragma unroll
        for (int w = 0; w < WT; ++w) live[w] = w < W ? (uint32_t)__builtin_amdgcn_readfirstlane((int)valid[q * W + w]) : 0u;
    } else {
        for (int w = tid; w < W; w += kBlock) live_l[w] = valid[q * W + w];
    }
    __syncthreads();
    // every round over the staged copy (S = true) or over global memory: two loops, so that no address is chosen between the two spaces
    auto rounds = [&](auto S) -> int {
    constexpr bool ST = decltype(S)::value;
    auto word = [&](int w, int i) -> uint32_t { if constexpr (ST) return stage[w * n_c + i]; else return mq[(u64)i * W + w]; };
    int t = 0;
    for (; t < max_picks; ++t) {
        u64 best = 0;
        int bidx = 0;
        for (int i = tid; i < n_c; i += kBlock) {
            int cnt = 0;
            if constexpr (WT > 0) {
#pragma unroll
                for (int w = 0; w < WT; ++w)
                    if (w < W) cnt += __popc(word(w, i) & live[w]);
            } else {
                for (int w = 0; w < W; ++w) cnt += __popc(word(w, i) & live_l[w]);
            }
            int rank;
            if constexpr (ST) rank = (int)stage[W * n_c + i]; else rank = cq[i].rank;
            const u64 key = ((u64)(uint32_t)cnt << 32) | (uint32_t)(0x7FFFFFFF - rank);      // greater count first, then the smaller rank
            if (key > best) { best = key; bidx = i; }
        }
#pragma unroll
        for (int s = kWave / 2; s > 0; s >>= 1) {
            const u64 ok = __shfl_xor(best, s);
            const int oi = __shfl_xor(bidx, s);
            if (ok > best) { best = ok; bidx = oi; }
        }
        if (lane == 0) { wkey[t & 1][wave] = best; widx[t & 1][wave] = bidx; }
        __syncthreads();
        best = wkey[t & 1][0]; bidx = widx[t & 1][0];
#pragma unroll
        for (int w = 1; w < kWavesPerBlock; ++w) {
            const u64 ok = wkey[t & 1][w];
            if (ok > best) { best = ok; bidx = widx[t & 1][w]; }
        }
        const int unique = __builtin_amdgcn_readfirstlane((int)(best >> 32));
        const int win = __builtin_amdgcn_readfirstlane(bidx);
        if (unique < c_min) break;                                           // (an empty segment: key 0)
        if constexpr (WT > 0) {
#pragma unroll
            for (int w = 0; w < WT; ++w)
                if (w < W) live[w] &= ~(uint32_t)__builtin_amdgcn_readfirstlane((int)word(w, win));
        } else {
            for (int w = tid; w < W; w += kBlock) live_l[w] &= ~word(w, win);
            __syncthreads();
        }
        if (tid == 0 && o.picks) {
            const GatherCand c = cq[win];
            o.picks[(u64)q * (u64)max_picks + (u64)t] = selhip_gather_pick_t{(int)q, c.rank, unique, c.count};
        }
    }
    return t;
    };
    const int t = staged ? rounds(std::true_type{}) : rounds(std::false_type{});
    if (tid == 0) {
        int left = 0;
        if constexpr (WT > 0) {
#pragma unroll
            for (int w = 0; w < WT; ++w) left += __popc(live[w]);
        } else {
            for (int w = 0; w < W; ++w) left += __popc(live_l[w]);
        }
        if (o.n_picks) o.n_picks[q] = t;
        if (o.unexplained) o.unexplained[q] = left;
    }
}

}  // namespace

// host_plan.hpp -- the decisions of the host side that are plain arithmetic, each written once: padding and grids, the shape of a
// signature build, the bit-plane count of a register range, which stage 1 a pass runs, the constants of the auxiliary criterion,
// the growth rule after an overflow and the units, slab and mirror rules of a dense matrix.  Nothing here touches the device or the context.
// Part of the kernel translation unit selection_kernels.hip (included there, before host_context.hpp); not a stand-alone header.
#pragma once

namespace {

bool is_pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }
int ilog2(int x) { int l = 0; while ((1 << l) < x) ++l; return l; }

// n rounded up to whole waves: the row pitch of the band-major signature layouts
template <typename T>
T pad_wave(T n) { return ((n + kWave - 1) / kWave) * kWave; }

unsigned grid_for(u64 items, unsigned per_block, unsigned max_blocks) {
    u64 b = (items + per_block - 1) / per_block;
    if (b < 1) b = 1;
    if (b > max_blocks) b = max_blocks;
    return (unsigned)b;
}

double relerr_scaled_for(int p) {
    // hll.h:662  relerr /= std::sqrt(m), relerr = 1e-2 (hll.h:211 default, :257)
    return 1e-2 / std::sqrt((double)(1ull << p));
}

// criteria_sketch.hpp:7-20 sigma(p): a double expression narrowed to float by the return type
float sigma_p_of(int p) {
    switch (p) {
        case 4: return (float)(1.106 / std::sqrt((double)(1 << p)));
        case 5: return (float)(1.07 / std::sqrt((double)(1 << p)));
        case 6: return (float)(1.054 / std::sqrt((double)(1 << p)));
        case 7: return (float)(1.046 / std::sqrt((double)(1 << p)));
    }
    return (float)(1.039 / std::sqrt((double)(1 << p)));
}

// what the kernels of the auxiliary-HLL criterion take for a precision p_aux.  One function for the all-pairs and the query passes, so
// the float / double roundings are the same in both
struct AuxConsts { double zs, S_sum, rs; };
AuxConsts aux_consts(int p_aux) {
    const float Z = 1.96f;                                   // z_score, selection.cpp:76
    const float zs_f = Z * sigma_p_of(p_aux);                // float * float (criteria_sketch.hpp:29,40)
    const double zs = (double)zs_f;
    return {zs, zs /* order_n = 1 (selection.cpp:77): S = Z*sigma_p */, relerr_scaled_for(p_aux)};
}

// ---- band shapes ------------------------------------------------------------------------------
bool stream_supported(int m, int n_rows) {
    return is_pow2(m) && m >= 128 && m <= 2048 && is_pow2(n_rows) && n_rows <= m;
}

bool sig_supported(int n_rows, int n_bands) {
    return is_pow2(n_rows) && (n_bands == 8 || n_bands == 16 || n_bands == 32 || n_bands == 64 || n_bands == 128);
}

// the tiled signature build (sig_build_tile_body) takes this band shape
bool sig_tile_shape(int m, int n_rows, int n_bands) {
    return is_pow2(m) && is_pow2(n_bands) && n_bands <= 128 && n_rows >= 2 && n_rows <= 32 && m >= 4;
}

// the grid of one signature build of n genomes: tiled (tile_g genomes per block, LDS transpose) for the shapes of the all-pairs joins
// unless "sig_tile" is off; one thread per bucket (tile_g = 0) otherwise
struct SigBuildShape { int tile_g; unsigned blocks; };
SigBuildShape sig_build_shape(int m, int n, int n_rows, int n_bands, int sig_tile, int sig_tile_g) {
    if (sig_tile && sig_tile_shape(m, n_rows, n_bands)) return {sig_tile_g, (unsigned)((n + sig_tile_g - 1) / sig_tile_g)};
    const long long threads = n_rows <= kWave ? (long long)n * m : (long long)n * n_bands;
    return {0, (unsigned)((threads + kBlock - 1) / kBlock)};
}

// bit planes that can be non-zero in a set whose largest register value is khi - 1: the NB of the stage-2a kernels
int bs_planes(int khi) { return khi <= 16 ? 4 : khi <= 32 ? 5 : 6; }

// the criterion has an auxiliary-HLL stage (hll_a, hll_an, hll_a + smh_a): it needs the auxiliary sketches
bool aux_criterion(int criterion) { return criterion == SELHIP_CRIT_HLL_A || criterion == SELHIP_CRIT_HLL_AN || criterion == SELHIP_CRIT_HLL_A_SMH_A; }
// stage 1's survivor list is the list stage 2 reads (smh_a, smh_c): nothing filters it again, and the survivors are the statistic
bool survivors_final(int criterion) { return criterion == SELHIP_CRIT_SMH_A || criterion == SELHIP_CRIT_SMH_C; }

// ---- which stage 1 a pass runs ------------------------------------------------------------------
// smh: the criterion has a stage 1 on the SuperMinHash rows that fills a survivor list -- smh_a alone or before hll_a, or the count of
// smh_c (hll_a / hll_an alone read neither the band shape nor the algorithm).  count: that stage is the count test of smh_c
// (kernel_smhc.cuh), which reads neither the band shape nor the algorithm either: none of the fields below is set.  use_sig: band
// signatures are built and joined (use_hash: by the sort join; use_index: a query pass probes the sorted index instead of joining);
// il_stream: ALGO_STREAM in its tiled form, which reads the bucket-interleaved copy of the sketches.  bad: the format of the error
// (it takes n_rows, n_bands) when the caller insisted on an algorithm that does not take the band shape.  emit: stage 1 emits the
// records -- the count under SELHIP_ESTIMATOR_SMH (selhip_ctx_set_estimator): the pass is its bounds or windows kernel, the count
// kernel and the counter copy; nothing is grouped, no histogram and no estimate is launched, no survivor list is filled
struct PassPlan {
    bool smh = false, count = false, emit = false, use_hash = false, use_sig = false, use_index = false, il_stream = false;
    const char* bad = nullptr;
};
PassPlan pass_plan(int criterion, int algo, int m, int n_rows, int n_bands, int estimator = SELHIP_ESTIMATOR_HLL) {
    PassPlan p;
    p.count = criterion == SELHIP_CRIT_SMH_C;
    p.emit = p.count && estimator == SELHIP_ESTIMATOR_SMH;
    p.smh = p.count || criterion == SELHIP_CRIT_SMH_A || criterion == SELHIP_CRIT_HLL_A_SMH_A;
    if (!p.smh || p.count) return p;
    const bool sig_ok = sig_supported(n_rows, n_bands);
    p.use_hash = algo == SELHIP_ALGO_HASHJOIN;
    p.use_index = algo == SELHIP_ALGO_INDEX;
    p.use_sig = p.use_hash || (algo != SELHIP_ALGO_STREAM && sig_ok);
    p.il_stream = !p.use_sig && stream_supported(m, n_rows);
    if (algo == SELHIP_ALGO_SIG && !sig_ok) p.bad = "ALGO_SIG needs power-of-two rows and 8..128 bands (got %d x %d)";
    else if (p.use_index && !sig_ok) p.bad = "ALGO_INDEX needs power-of-two rows and 8..128 bands (got %d x %d)";   // (no fallback: the caller asked for the index)
    else if (p.use_hash && (!is_pow2(n_rows) || n_bands > 65536)) p.bad = "ALGO_HASHJOIN needs power-of-two rows (got %d x %d)";
    return p;
}

// ---- after an overflow --------------------------------------------------------------------------
// The counts a pass reports are exact even when a list was too small, so the list grows once, to the count and an eighth, and the pass
// repeats; kMaxAttempts enqueues in all
constexpr int kMaxAttempts = 8;
size_t grown(u64 worst) { return (size_t)(worst + worst / 8 + 1024); }
// the result list: true (and its new capacity in *res_cap) when the pass selected more pairs than it holds
bool results_overflowed(u64 n_results, size_t have, size_t* res_cap) {
    if (n_results <= have) return false;
    *res_cap = grown(n_results);
    return true;
}

// ---- all-pairs top-k in row rounds (selhip_ctx_set_topk_rounds) ----------------------------------
// rows per round of a pass over n genomes: the setting itself, or under SELHIP_TOPK_ROUNDS_AUTO the largest R with R n <= 2^27 -- a round
// admits at most R n records, 2 GiB of them --, one row at least.  `period` (the rows after which the deal of a row interleave
// repeats, 1 without one): a round is whole periods, so that the rounds' rows are the rows the one-shot pass owns
constexpr long long kTopkRoundRecords = 1ll << 27;
long long topk_round_rows(long long setting, long long n, long long period) {
    long long r = setting > 0 ? setting : std::max<long long>(1, kTopkRoundRecords / std::max<long long>(1, n));
    return (r + period - 1) / period * period;
}

// pairs_direct_kernel: groups of four entries per wave and batch, and the grid -- one group per wave until the list has a group for
// every wave slot of the device (1 024 blocks of 8 waves), then up to 16
struct PairsDirectShape { int gpw; unsigned grid; };
PairsDirectShape pairs_direct_shape(u64 n_pairs) {
    const u64 slots = 1024ull * 8;
    const int gpw = (int)std::min<u64>(16, std::max<u64>(1, n_pairs / (4 * slots)));
    return {gpw, grid_for(n_pairs, 32u * (unsigned)gpw, 1024)};
}

// ---- dense matrices (kernel_matrix.cuh) -----------------------------------------------------------
// constexpr: the kernel reads the same rules (it is included behind this header).
// The units of a matrix of n_rows x n_cols cells: row tiles of four rows (one per wave) x spans of 64 columns, the spans dealt to
// the 8 XCD slots round robin as in dense_select_kernel -- unit u: slot u % 8, j = u / 8 -> row tile j % n_tiles of span 8 (j / n_tiles) + slot
constexpr int kMatrixSpan = kWave;
struct MatrixUnits { long long n_tiles, n_spans, n_units; };
// (tile_rows: the rows of a unit -- four, one per wave, for matrix_kernel; 4 Q, Q per wave, for the fast SuperMinHash kernel)
constexpr MatrixUnits matrix_units(long long n_rows, long long n_cols, int tile_rows = kWavesPerBlock) {
    const long long n_tiles = (n_rows + tile_rows - 1) / tile_rows, n_spans = (n_cols + kMatrixSpan - 1) / kMatrixSpan;
    return {n_tiles, n_spans, 8 * n_tiles * ((n_spans + 7) / 8)};
}
// a self matrix computes every pair once: row i of the slab [r0, r1) computes the columns [0, r0) u [i, n) ...
constexpr bool matrix_computes(int r0, int i, long long k) { return k < r0 || k >= i; }
// ... so it leaves out a span [k0, k0 + 64) that lies wholly under the diagonal and inside the slab ...
constexpr bool matrix_skips_span(int r0, int i, long long k0) { return k0 >= r0 && k0 + kMatrixSpan <= i; }
// ... and its cell (i, k) is also the cell (k, i) of a row of the same slab: stored twice
constexpr bool matrix_mirrors(int i, long long k, int r1) { return k > i && k < r1; }

// ---- long genomes split across workgroups (selhip_build_sketches_split, kernel_sketch.cuh) ---------
// The k-mer END positions of a genome of L codes are e in [k-1, L).  With a chunk length C (a positive multiple of kSketchSeg) chunk c
// owns e in [k-1 + c C, min(k-1 + (c+1) C, L)) and its kernel sees the sub-array codes + c C of length min(C + k-1, L - c C): the k-1
// warm-up bases of for_each_kmer are the real bases in front of the chunk, so every k-mer belongs to exactly one chunk and a window
// reset carries across a cut with no special case.  A genome has max(1, ceil((L - (k-1)) / C)) chunks and is split iff it has two.
constexpr long long kSplitChunkMin = (long long)kSketchSeg * 1024;     // auto never cuts below one stride of a 1 024-thread block
constexpr unsigned long long kSplitScratchMax = 1ull << 30;            // bytes of partial rows a call may hold (1 GiB)
// w: the rounds of resident blocks that auto aims at, C = max(kSplitChunkMin, round_up(end positions / (w B), kSplitChunkMin)).
// Not derivable from the code: chosen from the chunk sweep of scripts/bench_build_split.py (profiles/build_split_chunk_sweep.txt)
constexpr long long kSplitRounds = 1;

long long split_end_positions(long long L, int k) { return std::max<long long>(0, L - (k - 1)); }
long long split_chunks_of(long long L, int k, long long C) { return C > 0 ? std::max<long long>(1, (split_end_positions(L, k) + C - 1) / C) : 1; }
// bytes of partial rows per chunk: the main registers, the buckets, the auxiliary registers
unsigned long long split_row_bytes(int m, int p_aux) { return 16384ull + 8ull * (unsigned long long)std::max(m, 0) + (p_aux > 0 ? 1ull << p_aux : 0ull); }
// levels of the segmented reduction over c partial rows: no lane reduces more than SELHIP_MERGE_SEGMENT rows in sequence
int split_levels_of(long long c) {
    if (c < 2) return 0;
    int levels = 1;
    for (; c > SELHIP_MERGE_SEGMENT; ++levels) c = (c + SELHIP_MERGE_SEGMENT - 1) / SELHIP_MERGE_SEGMENT;
    return levels;
}

struct SplitPlan { long long chunk = 0, items = 0, split_genomes = 0, chunks = 0, max_chunks = 0; };
enum SplitPlanStatus { kSplitPlanOk = 0, kSplitPlanBadChunk, kSplitPlanBadOffsets, kSplitPlanScratch };

// The plan of one call: the chunk length and the chunks of every genome (counts[n], may be NULL).  chunk: SELHIP_SPLIT_OFF (nothing is
// split, the plan's chunk is 0), SELHIP_SPLIT_AUTO, or a positive multiple of kSketchSeg.  m, p_aux: of the rows asked for (0 = none):
// they size the scratch.  Auto raises C, doubling, until the partial rows fit kSplitScratchMax; an explicit chunk beyond it is refused.
SplitPlanStatus split_plan(const int64_t* off, int64_t n, int k, int m, int p_aux, int64_t chunk, int64_t resident_blocks, int64_t* counts, SplitPlan* out) {
    *out = SplitPlan{};
    if (chunk != SELHIP_SPLIT_OFF && chunk != SELHIP_SPLIT_AUTO && (chunk < 0 || chunk % kSketchSeg)) return kSplitPlanBadChunk;
    long long total = 0;
    for (int64_t g = 0; g < n; ++g) {
        if (off[g] < 0 || off[g + 1] < off[g]) return kSplitPlanBadOffsets;
        total += split_end_positions(off[g + 1] - off[g], k);
    }
    long long C = chunk == SELHIP_SPLIT_OFF ? 0 : chunk;
    if (chunk == SELHIP_SPLIT_AUTO) {
        const long long slots = kSplitRounds * std::max<long long>(1, resident_blocks);
        const long long per_slot = (total + slots - 1) / slots;
        C = std::max(kSplitChunkMin, (per_slot + kSplitChunkMin - 1) / kSplitChunkMin * kSplitChunkMin);
    }
    const unsigned long long row_bytes = split_row_bytes(m, p_aux);
    for (;;) {
        SplitPlan p;
        p.chunk = C;
        for (int64_t g = 0; g < n; ++g) {
            const long long c = split_chunks_of(off[g + 1] - off[g], k, C);
            if (c >= 2) { p.split_genomes += 1; p.chunks += c; p.items += c; p.max_chunks = std::max(p.max_chunks, c); }
            else p.items += 1;
        }
        if ((unsigned long long)p.chunks * row_bytes <= kSplitScratchMax) {
            for (int64_t g = 0; counts && g < n; ++g) counts[g] = split_chunks_of(off[g + 1] - off[g], k, C);
            *out = p;
            return kSplitPlanOk;
        }
        if (chunk != SELHIP_SPLIT_AUTO) return kSplitPlanScratch;
        C *= 2;
    }
}

// bit range of the band keys (band << 32 | signature) that the sort join and the query index sort
unsigned band_key_end_bit(int n_bands) { return 32u + (unsigned)ilog2(n_bands) + 1u; }

}  // namespace

// host_pass.hpp -- the pass scheduler of libselhip.so: kernel dispatch of stage 1 (stream / signature join / sort join), the
// auxiliary criteria, grouping, stage 2 (union histograms on bit planes or byte rows, estimator), chunk lanes, scratch sizing.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_context.hpp); not a stand-alone header.
#pragma once

namespace {

// ---- stage-1 dispatch ------------------------------------------------------------------------
template <int NCH, int LOG2R>
hipError_t launch_stream(selhip_ctx* c, const StageIO& io, const RowMap& rm) {
    constexpr int Q = kQueryVgprBudget / NCH;
    const int n = (int)c->n;
    const long long n_tiles_ll = rm.n_tiles(Q);
    if (n_tiles_ll > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const int n_tiles = (int)n_tiles_ll;
    // candidate columns that can matter: k in (row_begin, n)
    const int chunk_base = ((rm.row_begin + 1) / kChunk) * kChunk;
    const int n_chunks = (n - chunk_base + kChunk - 1) / kChunk;
    if (n_tiles <= 0 || n_chunks <= 0) return hipSuccess;
    const long long blocks = (long long)n_tiles * n_chunks;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL((smh_stream_kernel<NCH, LOG2R>), dim3((unsigned)blocks), dim3(kBlock), 0, io.st,
                       reinterpret_cast<const u64x2*>(c->aux_il.p), n, c->hi.p, c->pcb,
                       rm, n_tiles, chunk_base, io.surv, io.cap, io.pc);
    return hipGetLastError();
}

// LOG2R runs over 0 .. log2(m) = log2(128 * NCH)
template <int NCH, int LOG2R>
hipError_t launch_stream_r(selhip_ctx* c, const StageIO& io, int l, const RowMap& rm) {
    if (l == LOG2R) return launch_stream<NCH, LOG2R>(c, io, rm);
    if constexpr ((1 << LOG2R) < 128 * NCH) return launch_stream_r<NCH, LOG2R + 1>(c, io, l, rm);
    return hipErrorInvalidValue;
}

hipError_t launch_stage1(selhip_ctx* c, const StageIO& io, int n_rows, int n_bands, const RowMap& rm) {
    if (stream_supported(c->m, n_rows)) {
        const int nch = c->m / 128;
        const int l = ilog2(n_rows);
        switch (nch) {
            case 1: return launch_stream_r<1, 0>(c, io, l, rm);
            case 2: return launch_stream_r<2, 0>(c, io, l, rm);
            case 4: return launch_stream_r<4, 0>(c, io, l, rm);
            case 8: return launch_stream_r<8, 0>(c, io, l, rm);
            case 16: return launch_stream_r<16, 0>(c, io, l, rm);
        }
    }
    const long long rows = rm.n_tiles(1);
    const int n = (int)c->n;
    const int chunks = (n + kBlock - 1) / kBlock;
    const long long blocks = rows * chunks;
    if (blocks <= 0) return hipSuccess;
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    hipLaunchKernelGGL(smh_generic_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, io.st,
                       c->d_aux, n, c->m, n_rows, n_bands, c->hi.p, c->pcb, rm, (int)rows,
                       io.surv, io.cap, io.pc);
    return hipGetLastError();
}

// ---- stage 1 of criterion smh_c (kernel_smhc.cuh) -----------------------------------------------
// the passes under the criterion apply the containment rule (selhip_ctx_set_min_containment) on top of c_min
bool smhc_containment(const selhip_ctx* c) { return !std::isnan(c->min_containment); }
// what SELHIP_CRIT_SMH_C asks of the context, checked by every entry before it claims a counter set
int accept_count(selhip_ctx* c) {
    if (c->m <= 0 || (!c->d_aux && c->n)) { set_err(&c->err, "criterion smh_c (SELHIP_CRIT_SMH_C) needs SuperMinHash rows: the context holds none"); return SELHIP_E_BADARG; }
    if (c->min_matches < 1 && !smhc_containment(c)) { set_err(&c->err, "criterion smh_c (SELHIP_CRIT_SMH_C) needs a count threshold: selhip_ctx_set_min_matches (a fixed c_min) or selhip_ctx_set_min_containment (a per-pair one) first"); return SELHIP_E_BADARG; }
    if (c->min_matches > c->m) { set_err(&c->err, "criterion smh_c (SELHIP_CRIT_SMH_C): c_min = %d exceeds the m = %d buckets of a row", c->min_matches, c->m); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

// ---- the measure of the passes (selhip_ctx_set_measure) ------------------------------------------
// what SELHIP_MEASURE_MAX_CONTAINMENT refuses, checked by every entry before it claims a counter set: the CB bound and the auxiliary-HLL
// criteria are bounds on J -- e_small / e_large >= tau is necessary for J >= tau, not for I / e_small >= tau -- and would silently drop
// the pairs of unequal size that the measure exists for.  (smh_a and smh_c test bucket equality, not J: the caller's choice.)
int accept_measure(selhip_ctx* c, int mode) {
    if (c->measure == SELHIP_MEASURE_JACCARD) return SELHIP_OK;
    if (mode == SELHIP_MODE_CB_SMH) {
        set_err(&c->err, "measure max_containment (SELHIP_MEASURE_MAX_CONTAINMENT) takes no SELHIP_MODE_CB_SMH: the CB bound is a bound on J and "
                         "cuts pairs of unequal size; pass SELHIP_MODE_SMH");
        return SELHIP_E_BADARG;
    }
    if (aux_criterion(c->criterion)) {
        set_err(&c->err, "measure max_containment (SELHIP_MEASURE_MAX_CONTAINMENT) takes no auxiliary-HLL criterion (criterion %d: hll_a, hll_an "
                         "and hll_a + smh_a bound J); use smh_a, smh_c or none", c->criterion);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

// ---- the estimator of the records (selhip_ctx_set_estimator) -------------------------------------
// what SELHIP_ESTIMATOR_SMH refuses, checked by every entry before it claims a counter set: the estimate is a function of the count of
// equal buckets, which criterion smh_c alone computes for every pair it admits
int accept_estimator(selhip_ctx* c) {
    if (c->estimator == SELHIP_ESTIMATOR_HLL || c->criterion == SELHIP_CRIT_SMH_C) return SELHIP_OK;
    set_err(&c->err, "estimator smh (SELHIP_ESTIMATOR_SMH) records a value computed from the count of criterion smh_c (SELHIP_CRIT_SMH_C) and "
                     "takes no other criterion (criterion %d); selhip_ctx_set_estimator(ctx, SELHIP_ESTIMATOR_HLL) first", c->criterion);
    return SELHIP_E_BADARG;
}
// what selhip_ctx_set_topk_rounds asks of an all-pairs pass, checked before it claims a counter set: the rounds prune at the source with
// the value the count kernel computes, and what they carry is the all-pairs top-k
int accept_rounds(selhip_ctx* c) {
    if (c->topk_rounds == 0) return SELHIP_OK;
    if (c->allpairs_topk > 0 && c->criterion == SELHIP_CRIT_SMH_C && c->estimator == SELHIP_ESTIMATOR_SMH) return SELHIP_OK;
    set_err(&c->err, "row rounds (selhip_ctx_set_topk_rounds) are for all-pairs top-k passes (selhip_ctx_set_allpairs_topk: %d) of criterion smh_c "
                     "(SELHIP_CRIT_SMH_C) under the estimator smh (SELHIP_ESTIMATOR_SMH) (criterion %d, estimator %d); "
                     "selhip_ctx_set_topk_rounds(ctx, 0) first", c->allpairs_topk, c->criterion, c->estimator);
    return SELHIP_E_BADARG;
}
// what the count kernels of a pass that emits take besides: its records go to the context's result list behind block 0's n_results.
// (the count floor of such a pass is 1: a pair without an equal bucket has no record)
SmhcEmit smhc_emit(const selhip_ctx* c, PassCounters* pc0) { return SmhcEmit{(double)c->tau_f, c->measure, pc0}; }
int smhc_floor(const selhip_ctx* c) { return c->plan.emit ? std::max(c->min_matches, 1) : c->min_matches; }

// the rows of X (owned rows of rm) against the candidates of Y from first_cand on.  QUERY = false: X = Y = the context's rows, windows
// from hi and pc_in's z0; QUERY = true: the queries against the database, windows lo / hi
// (ex, ey: the truncated cardinalities of the rows and of the candidates, read by the containment rule alone)
struct CountSets { const u64* X; const u64* Y; int n_x, n_y; const int* lo; const int* hi; const PassCounters* pc_in; const u64* ex; const u64* ey; };
// pc0 (a pass that emits, else null): the pass's counter block 0 -- the records go to the context's result list, `surv` is not written
// and pc->n_survivors takes the tally of the pairs that passed the count test
template <bool QUERY>
hipError_t launch_count(selhip_ctx* c, hipStream_t st, const CountSets& a, const RowMap& rm, int first_cand,
                        selhip_int2_t* surv, u64 cap, PassCounters* pc, PassCounters* pc0 = nullptr) {
    const int m = c->m, c_min = smhc_floor(c);
    const bool emit = pc0 != nullptr;
    selhip_pair_t* const res = c->results.p;
    const u64 res_cap = (u64)c->results.cap;
    c->smhc_path_used = smhc_fast(m) ? 1 : 0;
    const bool cont = smhc_containment(c);
    c->smhc_rule_used = cont ? 1 : 0;
    const SmhcRule rule{c->min_containment, a.ex, a.ey};
    const SmhcRuleEmit rule_em{rule, smhc_emit(c, pc0)};
    // a round of a top-k pass in row rounds: the TOPK form, whose operand rides behind the emit form's
    const bool topk = !QUERY && emit && c->rd.on;
    const SmhcRuleEmitTopk rule_tk{rule_em, c->topk_thr.p};
    if (smhc_fast(m)) {
        const int nch = m / 128;
        const long long n_tiles = rm.n_tiles(smhc_q(nch, smhc_tight(emit, cont, topk)));
        if (n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
        const int chunk_base = (first_cand / kChunk) * kChunk;
        const int n_chunks = (a.n_y - chunk_base + kChunk - 1) / kChunk;
        if (n_tiles <= 0 || n_chunks <= 0) return hipSuccess;
        const long long blocks = n_tiles * n_chunks;
        if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
#define SELHIP_SMHC_LAUNCH_R(NCH, RULE) do { \
            if constexpr (!QUERY) if (topk) { \
                hipLaunchKernelGGL((smh_count_kernel<NCH, false, RULE, true, true>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const u64x2*)a.X, (const u64x2*)a.Y, \
                                   a.n_x, a.n_y, a.lo, a.hi, a.pc_in, rm, (int)n_tiles, chunk_base, c_min, res, res_cap, pc, rule_tk); \
                break; } \
            if (emit) hipLaunchKernelGGL((smh_count_kernel<NCH, QUERY, RULE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const u64x2*)a.X, (const u64x2*)a.Y, \
                                         a.n_x, a.n_y, a.lo, a.hi, a.pc_in, rm, (int)n_tiles, chunk_base, c_min, res, res_cap, pc, rule_em); \
            else hipLaunchKernelGGL((smh_count_kernel<NCH, QUERY, RULE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, st, (const u64x2*)a.X, (const u64x2*)a.Y, \
                                    a.n_x, a.n_y, a.lo, a.hi, a.pc_in, rm, (int)n_tiles, chunk_base, c_min, surv, cap, pc, rule); } while (0)
#define SELHIP_SMHC_LAUNCH(NCH) do { if (cont) SELHIP_SMHC_LAUNCH_R(NCH, kSmhcContainment); else SELHIP_SMHC_LAUNCH_R(NCH, kSmhcFixed); } while (0)
        switch (nch) {
            case 1: SELHIP_SMHC_LAUNCH(1); break;
            case 2: SELHIP_SMHC_LAUNCH(2); break;
            case 4: SELHIP_SMHC_LAUNCH(4); break;
            default: SELHIP_SMHC_LAUNCH(8);
        }
#undef SELHIP_SMHC_LAUNCH
#undef SELHIP_SMHC_LAUNCH_R
        return hipGetLastError();
    }
    const long long rows = rm.n_tiles(1);
    const long long blocks = rows * ((a.n_y + kBlock - 1) / kBlock);
    if (blocks <= 0) return hipSuccess;
    if (rows > 0x7FFFFFFFll || blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    with_flag(cont, [&](auto C) {
        constexpr int RULE = decltype(C)::value ? kSmhcContainment : kSmhcFixed;
        if constexpr (!QUERY) {
            if (topk) {
                hipLaunchKernelGGL((smh_count_generic_kernel<false, RULE, true, true>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a.X, a.Y, a.n_x, a.n_y, m, a.lo, a.hi, a.pc_in,
                                   rm, (int)rows, c_min, res, res_cap, pc, rule_tk);
                return;
            }
        }
        if (emit)
            hipLaunchKernelGGL((smh_count_generic_kernel<QUERY, RULE, true>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a.X, a.Y, a.n_x, a.n_y, m, a.lo, a.hi, a.pc_in,
                               rm, (int)rows, c_min, res, res_cap, pc, rule_em);
        else
            hipLaunchKernelGGL((smh_count_generic_kernel<QUERY, RULE, false>), dim3((unsigned)blocks), dim3(kBlock), 0, st, a.X, a.Y, a.n_x, a.n_y, m, a.lo, a.hi, a.pc_in,
                               rm, (int)rows, c_min, surv, cap, pc, rule);
    });
    return hipGetLastError();
}

// the all-pairs form behind cb_bounds_kernel: candidates k > row_begin, as in launch_stage1
hipError_t launch_stage1_count(selhip_ctx* c, const StageIO& io, const RowMap& rm) {
    const int n = (int)c->n;
    return launch_count<false>(c, io.st, CountSets{c->d_aux, c->d_aux, n, n, nullptr, c->hi.p, c->pcb, c->ecard.p, c->ecard.p}, rm, rm.row_begin + 1, io.surv, io.cap, io.pc,
                               c->plan.emit ? c->pcb : nullptr);
}


// pairs of the all-pairs triangle that this context's passes cover
double join_pairs_here(const selhip_ctx* c) {
    return 0.5 * (double)c->n * (double)c->n / std::max(1, c->il_parts);
}

// tile height of the signature joins: the configured one, or the automatic choice (see selhip_ctx::join_qt)
int join_tile_rows(const selhip_ctx* c) {
    const double pairs_here = join_pairs_here(c);
    // (< 1e8 pairs: 32-row tiles -- twice the work units for the 8 192 wave slots, a shorter tail: cfg3's join 108.5 -> 104.3 us)
    // (the sliced join kept these heights: cfg3 32 / 64 rows 239.7 / 239.2 us a pass, cfg4 64 / 128 rows 1643 / 1633 us at T = 1,
    //  profiles/join_sliced_sweep.txt)
    int qt = c->join_qt > 0 ? c->join_qt : (pairs_here >= 4.5e8 ? 128 : pairs_here >= 2e8 ? 64 : 32);      // (one of 8 ranks of cfg4, 1.6e8 pairs: 32 rows 0.450 ms, 64 rows 0.481)
    if (c->il_parts > 1) { qt = std::min(qt, c->il_block); while (c->il_block % qt) qt -= 16; }
    return qt;
}

// the grid of a signature join: tiles of qt query rows x blocks of gpb candidate groups (a group = 64 candidates, one wave's worth),
// the candidates being k > row_begin, k >= cand_begin.  blocks = 0: nothing to launch.  nd > 0: the join reads nd dwords per genome
// through 32-bit offsets into a band-major signature array of pitch n_pad, which must therefore stay below 2 GiB
struct JoinGeometry { int n_tiles, group_base, n_gblocks; long long blocks; };
hipError_t join_geometry(const selhip_ctx* c, const RowMap& rm, int qt, int gpb, int nd, int n_pad, JoinGeometry* g) {
    if ((long long)nd * n_pad * 4 >= (1ll << 31)) return hipErrorInvalidValue;
    const long long n_tiles_ll = rm.n_tiles(qt);
    if (n_tiles_ll > 0x7FFFFFFFll) return hipErrorInvalidValue;
    g->n_tiles = (int)n_tiles_ll;
    g->group_base = (std::max(rm.row_begin + 1, (int)c->cand_begin) / kWave / gpb) * gpb;
    const int n_groups = ((int)c->n + kWave - 1) / kWave - g->group_base;
    g->n_gblocks = (n_groups + gpb - 1) / gpb;
    g->blocks = g->n_tiles <= 0 || g->n_gblocks <= 0 ? 0 : (long long)g->n_tiles * g->n_gblocks;
    return g->blocks > 0x7FFFFFFFll ? hipErrorInvalidValue : hipSuccess;
}

template <int NB>
hipError_t launch_join(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    const int qt = join_tile_rows(c);   // query rows per block (multiple of 16)
    JoinGeometry g;
    const hipError_t e = join_geometry(c, rm, qt, kWavesPerBlock, 0, n_pad, &g);
    if (e != hipSuccess || g.blocks == 0) return e;
    hipLaunchKernelGGL((sig_join_kernel<NB>), dim3((unsigned)g.blocks), dim3(kBlock), 0, io.st,
                       c->sig.T.p, (int)c->n, n_pad, c->hi.p, c->pcb, rm, g.n_tiles, g.group_base, qt,
                       io.cand, io.cap, io.pc);
    return hipGetLastError();
}

template <int ND, bool DB, int WPB>
hipError_t launch_join16_w(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    const int qt = join_tile_rows(c);
    JoinGeometry g;
    const hipError_t e = join_geometry(c, rm, qt, WPB, ND, n_pad, &g);
    if (e != hipSuccess || g.blocks == 0) return e;
    hipLaunchKernelGGL((sig16_join_kernel<ND, DB, WPB>), dim3((unsigned)g.blocks), dim3(WPB * kWave), 0, io.st,
                       c->sig.P.p, (int)c->n, n_pad, c->hi.p, c->pcb, rm, g.n_tiles, g.group_base, qt,
                       io.cand, io.cap, io.seg_cnt);
    return hipGetLastError();
}

// the all-pairs join of this band shape runs on bit-sliced signatures ("join_form" = 2: the LDS-tile 16-bit join, and a tiled build to
// write the layout; any other shape keeps the packed form 0).  The build and the join both ask, so they always agree on the layout.
bool join_sliced(const selhip_ctx* c, int n_rows, int n_bands) {
    return c->join_form == 2 && c->join_bits == 16 && c->join_q && c->algo != SELHIP_ALGO_HASHJOIN && c->sig_tile && sig_tile_shape(c->m, n_rows, n_bands);
}

template <int ND, int T, int WPB, int FORM>
hipError_t launch_joinl_w(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    const int n = (int)c->n;
    // tile height: the configured one, capped so that the tile (+ appenders) fits 64 KiB of LDS; a multiple of 16 that divides the
    // interleave block when rows are interleaved
    int qt = std::min(join_tile_rows(c), (int)((64 * 1024 - WPB * kAppendCap * sizeof(selhip_int2_t)) / (ND * 4 + 4) - kJoinTilePadRows) / 16 * 16);
    if (c->il_parts > 1) while (c->il_block % qt) qt -= 16;
    constexpr int GPB = WPB * T;                                                          // candidate groups per block
    JoinGeometry g;
    const hipError_t e = join_geometry(c, rm, qt, GPB, ND, n_pad, &g);
    if (e != hipSuccess || g.blocks == 0) return e;
    const int n_tiles = g.n_tiles, group_base = g.group_base, n_gblocks = g.n_gblocks;
    long long blocks = g.blocks;
    // only the units above the diagonal (JoinTriangle, kernel_sigjoin.cuh) when the rows are contiguous and the tiles line up with the
    // 256-candidate blocks; otherwise the rectangle, whose blocks under the diagonal leave at once
    JoinTriangle tri{0, 0, 0, 0};
    constexpr int kCand = GPB * kWave;
    if (c->join_tri && rm.n_parts == 1 && kCand % qt == 0 && rm.row_begin % qt == 0 && blocks < 0x7FFFFFFFll) {
        const int a = kCand / qt, g_lo = group_base / GPB, rbq = rm.row_begin / qt;
        const long long c0 = (long long)a * (g_lo + 1) - rbq;
        if (c0 >= 1) {
            // columns k = 0 .. K-1 hold c0 + a k < n_tiles units
            long long K = c0 >= n_tiles ? 0 : ((long long)n_tiles - c0 + a - 1) / a;
            K = std::min<long long>(K, n_gblocks);
            const long long SK = K * c0 + (long long)a * K * (K - 1) / 2;
            const long long total = SK + (long long)(n_gblocks - K) * n_tiles;
            if (total > 0 && total < 0x7FFFFFFFll) { tri = JoinTriangle{a, (int)c0, (int)K, (int)SK}; blocks = total; }
        }
    }
    if (blocks > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const size_t smem = (size_t)WPB * kAppendCap * sizeof(selhip_int2_t) + (size_t)((qt + 3) & ~3) * 4 + (size_t)(qt + kJoinTilePadRows) * ND * 4;
    if (smem > 64 * 1024) return hipErrorInvalidValue;                                   // join_qt is capped so that this cannot happen
    hipLaunchKernelGGL((sigl_join_kernel<ND, T, WPB, FORM>), dim3((unsigned)blocks), dim3(WPB * kWave), smem, io.st,
                       c->sig.P.p, c->sig.G.p, n, n_pad, c->hi.p, c->pcb, rm, n_tiles, group_base, qt,
                       io.cand, io.cap, io.seg_cnt, c->mode == SELHIP_MODE_CB_SMH ? 1 : 0, tri);
    return hipGetLastError();
}

// (T = 2 groups of candidates per wave -- half the LDS reads -- was measured twice with the packed minimum: 130 VGPRs, 3 waves per SIMD,
// cfg3 157 vs 127 us, cfg4 2.37 vs 2.07 ms; and, after the wait counts left the row loop, capped at 128 VGPRs / 4 waves per SIMD: cfg3
// 121 vs 101 us, cfg4 2.28 vs 2.02 ms -- that loop wants waves, not fewer LDS reads.  The sliced loop issues a third of the instructions
// per row, so it is built with T = 2 as well (nb <= 64, where 2 x ND candidate registers fit in 128 VGPRs).  Measured (three rounds,
// profiles/join_sliced_sweep.txt): cfg3 T = 2 241.9 vs T = 1 239.7 us a pass, cfg4 1525 vs 1633 us -- at the pass sizes that take
// 128-row tiles (>= 4.5e8 pairs) the halved LDS reads pay, below they do not: "join_t" = 0 (automatic) picks T by that size.)
template <int ND, int FORM>
hipError_t launch_joinl_f(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    const int t = c->join_t ? c->join_t : join_pairs_here(c) >= 4.5e8 ? 2 : 1;
    if constexpr (FORM == 3 && ND <= 32)
        if (t == 2) return c->join_wpb == 8 ? launch_joinl_w<ND, 2, 8, FORM>(c, io, n_pad, rm) : launch_joinl_w<ND, 2, 4, FORM>(c, io, n_pad, rm);
    return c->join_wpb == 8 ? launch_joinl_w<ND, 1, 8, FORM>(c, io, n_pad, rm) : launch_joinl_w<ND, 1, 4, FORM>(c, io, n_pad, rm);
}

// kernel FORM of sigl_join_kernel: 1 = 15-bit flags, 3 = bit-sliced ("join_form" 2), 2 = zero-half ("join_form" 1), 0 = packed minimum
template <int ND>
hipError_t launch_joinl(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    if (c->join_bits == 15) { c->join_form_used = 1; return launch_joinl_f<ND, 1>(c, io, n_pad, rm); }
    if (join_sliced(c, c->n_rows, c->n_bands)) { c->join_form_used = 3; return launch_joinl_f<ND, 3>(c, io, n_pad, rm); }
    if (c->join_form == 1) { c->join_form_used = 2; return launch_joinl_f<ND, 2>(c, io, n_pad, rm); }
    c->join_form_used = 0;
    return launch_joinl_f<ND, 0>(c, io, n_pad, rm);
}

template <int ND, bool DB>
hipError_t launch_join16(selhip_ctx* c, const StageIO& io, int n_pad, const RowMap& rm) {
    if (c->join_q) return launch_joinl<ND>(c, io, n_pad, rm);
    c->join_form_used = -1;
    return c->join_wpb == 1 ? launch_join16_w<ND, DB, 1>(c, io, n_pad, rm) : launch_join16_w<ND, DB, 4>(c, io, n_pad, rm);
}

// what sig_build_kernel takes besides the sketches and the arrays it writes.  The defaults are the build alone: no bounds blocks, 16-bit
// pairs packed (never sliced) in P / G -- the database's signatures of the query passes, whatever "join_bits" and "join_form" say
struct SigBuildPass {
    unsigned work_blocks;
    int bounds_blocks = 0;
    const double* cards = nullptr; double tau = 0.0; int use_cb = 0; RowMap rm{0, 0, 1, 1, 0};
    u64* ecard = nullptr; int* hi = nullptr; PassCounters* pc = nullptr;
    int* csr_cnt = nullptr; int csr_cap = 0; int cand_begin = 0;
    u64* seg_cnt = nullptr; int seg_cap = 0;
    int pk_shift = 16;
    PassCounters* zero_pc = nullptr;
    int slice = 0;
};

// band signatures of the context's sketches in the band shape (n_rows, n_bands) into the four layouts of `s`
hipError_t launch_sig_kernel(selhip_ctx* c, SigSet& s, int n_rows, int n_bands, const SigBuildShape& sh, const SigBuildPass& a) {
    const int n = (int)c->n;
    if (a.work_blocks + (unsigned)a.bounds_blocks == 0) return hipSuccess;
    hipLaunchKernelGGL(sig_build_kernel, dim3(a.work_blocks + (unsigned)a.bounds_blocks), dim3(kBlock), 0, c->stream,
                       c->d_aux, n, c->m, n_rows, n_bands, pad_wave(n), s.Q.p, s.T.p, s.P.p, s.G.p,
                       a.bounds_blocks, a.cards, a.tau, a.use_cb, a.rm, a.ecard, a.hi, a.pc, a.csr_cnt, a.csr_cap, a.cand_begin,
                       a.seg_cnt, a.seg_cap, a.pk_shift, a.zero_pc, sh.tile_g, a.slice);
    return hipGetLastError();
}

// what the context's signature arrays hold after a build for this band shape under the current settings (never 0): the "sig_cache" key
long long sig_cache_key(const selhip_ctx* c, int n_rows, int n_bands) {
    const SigBuildShape sh = sig_build_shape(c->m, (int)c->n, n_rows, n_bands, c->sig_tile, c->sig_tile_g);
    return ((long long)n_rows << 40) | ((long long)n_bands << 20) | ((long long)join_sliced(c, n_rows, n_bands) << 3) | ((long long)(c->join_bits == 15) << 2) |
           (sh.tile_g ? 2 : 0) | 1;
}

// the all-pairs pass's build of the context's own signatures, with the pass's bounds computation riding in its first blocks
hipError_t launch_sig_build(selhip_ctx* c, int n_rows, int n_bands, double tau, int rb, int re, PassCounters* zero_pc) {
    const int n = (int)c->n;
    TimerScope t(c, T_SIGBUILD);
    const SigBuildShape sh = sig_build_shape(c->m, n, n_rows, n_bands, c->sig_tile, c->sig_tile_g);
    const bool slice = join_sliced(c, n_rows, n_bands);                  // sig.P / sig.G bit-sliced instead of packed
    // "sig_cache": the signatures depend on the sketches and the band shape only, so a context that runs many passes over the same
    // sketches (the ranks of a strong-scaled job, a threshold sweep) builds them once; upload / attach and any reallocation of the
    // signature arrays invalidate them.  The bounds blocks still run every pass (they depend on tau, the mode and the rows).  The key
    // holds the layout of sigP / sigG (15-bit, 16-bit packed or sliced), so a join never reads words written for another.
    const long long sig_key = sig_cache_key(c, n_rows, n_bands);
    const bool cached = c->sig_cache && c->sig_key == sig_key;
    c->sig_key = c->sig_cache ? sig_key : 0;
    const SigBuildPass a{cached ? 0u : sh.blocks, (n + kBlock - 1) / kBlock,
                         c->d_cards, tau, c->mode == SELHIP_MODE_CB_SMH ? 1 : 0, row_map(c, rb, re), c->ecard.p, c->hi.p, c->pcb,
                         grouping_on(c) ? c->csr_cnt.p : nullptr, grouping_on(c) ? (int)c->csr_cnt.cap : 0, (int)c->cand_begin,
                         c->seg_cnt.p, (int)c->seg_cnt.cap, c->join_bits == 15 ? 17 : 16, zero_pc, slice ? 1 : 0};
    return launch_sig_kernel(c, c->sig, n_rows, n_bands, sh, a);
}

// signature join + exact verification of the query rows [rb, re) (sig_build must have run)
hipError_t launch_stage1_sig(selhip_ctx* c, const StageIO& io, int n_rows, int n_bands, const RowMap& rm) {
    const int n = (int)c->n;
    const int n_pad = pad_wave(n);
    hipError_t e = hipSuccess;
    if (c->join_bits == 16 || c->join_bits == 15) {
        {
            TimerScope t(c, T_JOIN, io.st);
            switch (n_bands) {
                case 8: e = c->join_db ? launch_join16<4, true>(c, io, n_pad, rm) : launch_join16<4, false>(c, io, n_pad, rm); break;
                case 16: e = c->join_db ? launch_join16<8, true>(c, io, n_pad, rm) : launch_join16<8, false>(c, io, n_pad, rm); break;
                case 32: e = c->join_db ? launch_join16<16, true>(c, io, n_pad, rm) : launch_join16<16, false>(c, io, n_pad, rm); break;
                case 64: e = c->join_db ? launch_join16<32, true>(c, io, n_pad, rm) : launch_join16<32, false>(c, io, n_pad, rm); break;
                case 128: e = c->join_db ? launch_join16<64, true>(c, io, n_pad, rm) : launch_join16<64, false>(c, io, n_pad, rm); break;
                default: return hipErrorInvalidValue;
            }
        }
        if (e != hipSuccess) return e;
        // the 16-bit matches were staged in the candidate list; survivors go to the survivor list as usual
        TimerScope t(c, T_VERIFY, io.st);
        static_assert(1024 % kAppendSegs == 0, "verify16_kernel: the grid is a multiple of the segment count");
        hipLaunchKernelGGL(verify16_kernel, dim3(1024), dim3(kVerifyBlock), 0, io.st, c->d_aux, c->m, n_rows, n_bands, c->sig.Q.p,
                           io.cand, io.seg_cnt, io.cap, io.surv, io.cap, io.pc, c->verify_fb, io.row_cnt, io.row_lab, n);
        return hipGetLastError();
    } else {
        TimerScope t(c, T_JOIN, io.st);
        switch (n_bands) {
            case 8: e = launch_join<8>(c, io, n_pad, rm); break;
            case 16: e = launch_join<16>(c, io, n_pad, rm); break;
            case 32: e = launch_join<32>(c, io, n_pad, rm); break;
            case 64: e = launch_join<64>(c, io, n_pad, rm); break;
            case 128: e = launch_join<128>(c, io, n_pad, rm); break;
            default: return hipErrorInvalidValue;
        }
    }
    if (e != hipSuccess) return e;
    TimerScope t(c, T_VERIFY, io.st);
    hipLaunchKernelGGL(verify_kernel, dim3(1024), dim3(kBlock), 0, io.st, c->d_aux, c->m, n_rows, n_bands,
                       io.cand, &io.pc->n_candidates, io.cap, io.surv, io.cap, io.pc);
    return hipGetLastError();
}

// the keys (band << 32 | signature) and ranks of n genomes from their band-major signatures sigT, then sorted by key (rocPRIM) into
// keys_out / vals_out; tmp holds tmp_bytes of rocPRIM's temporary storage (sized by a radix_sort_pairs call with a null pointer)
hipError_t sort_band_keys(hipStream_t st, const uint32_t* sigT, int n, int n_bands, u64* keys_in, u64* keys_out, int* vals_in, int* vals_out,
                          char* tmp, size_t tmp_bytes) {
    const size_t total = (size_t)n * n_bands;
    hipLaunchKernelGGL(sigkey_build_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, st,
                       sigT, n, pad_wave(n), n_bands, keys_in, vals_in);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    return rocprim::radix_sort_pairs(tmp, tmp_bytes, keys_in, keys_out, vals_in, vals_out, total, 0u, band_key_end_bit(n_bands), st);
}

// sort-based join of the band signatures (sig_build must have run); rows [rb, re)
hipError_t launch_stage1_hashjoin(selhip_ctx* c, const StageIO& io, int n_rows, int n_bands, const RowMap& rm) {
    const int n = (int)c->n;
    const long long total = (long long)n * n_bands;
    if (total <= 0) return hipSuccess;
    TimerScope t(c, T_JOIN, io.st);
    const hipError_t e = sort_band_keys(io.st, c->sig.T.p, n, n_bands, c->hj_keys_in.p, c->hj_keys_out.p, c->hj_vals_in.p, c->hj_vals_out.p,
                                        c->hj_tmp.p, c->hj_tmp.cap);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(run_emit_kernel, dim3(grid_for((u64)total, kBlock, 8192)), dim3(kBlock), 0, io.st,
                       c->hj_keys_out.p, c->hj_vals_out.p, total, c->sig.Q.p, n_bands, c->d_aux, c->m, n_rows, n_bands,
                       n, c->hi.p, c->pcb, rm, io.surv, io.cap, io.pc);
    return hipGetLastError();
}

template <int MODE>
hipError_t launch_select(bool fma, hipStream_t st, unsigned grid, const uint32_t* counts, const u64* n_dev, u64 n_host,
                         u64 cap, int p, double* est, const selhip_int2_t* pairs, const u64* ecard, double tau,
                         selhip_pair_t* results, u64 results_cap, PassCounters* pc,
                         selhip_result_t* rf32, int* out_count, u64 chunk_off = 0, u64 chunk_len = ~0ull, int measure = SELHIP_MEASURE_JACCARD) {
    const double rs = relerr_scaled_for(p);
    // (the measure of a pass is a template argument: under J the kernel is the one it always was)
    with_flag(fma, [&](auto F) {
        auto launch = [&](auto M) {
            hipLaunchKernelGGL((ertl_select_kernel<decltype(F)::value, MODE, decltype(M)::value>), dim3((grid + kWavesPerBlock - 1) / kWavesPerBlock), dim3(kBlock), 0, st, counts, n_dev, n_host, cap,
                               p, rs, est, pairs, ecard, tau, results, results_cap, pc, rf32, out_count, chunk_off, chunk_len);
        };
        if constexpr (MODE == 1) {                                           // (the selecting form alone has a measure)
            if (measure == SELHIP_MEASURE_MAX_CONTAINMENT) { launch(std::integral_constant<int, SELHIP_MEASURE_MAX_CONTAINMENT>{}); return; }
        }
        launch(std::integral_constant<int, SELHIP_MEASURE_JACCARD>{});
    });
    return hipGetLastError();
}

// ---- stage 2a on bit planes (kernel_hllbs.cuh) -------------------------------------------------
// the instantiation for a set whose largest register value is khi - 1 = the number of bit planes that can be non-zero; sparse_t = 0:
// every value decoded from the planes, else the set's sparse threshold (a multiple of 4 in [4, kBsSparseMaxT]) with its lists
template <int NB>
void launch_hist_bs_nb(int g1, unsigned blocks, hipStream_t st, const uint32_t* bs, const uint8_t* gmax, const uint32_t* lists, const selhip_int2_t* list,
                       const u64* count, u64 cap, uint32_t* counts, u64 off, u64 window, int run, u64 dense_pairs) {
#define SELHIP_BS_LAUNCH(G1) hipLaunchKernelGGL((hll_union_hist_bs_kernel<NB, G1>), dim3(blocks), dim3(kBlock), 0, st, bs, gmax, lists, list, count, cap, \
                                                counts, off, window, run, dense_pairs)
    switch (g1) {
        case 1: SELHIP_BS_LAUNCH(1); return;
        case 2: SELHIP_BS_LAUNCH(2); return;
        case 3: SELHIP_BS_LAUNCH(3); return;
    }
    // (four planes hold values < 16: a threshold of 16 or more leaves every list empty.  With five planes G1 = 6 would spill -- 128
    //  VGPRs and scratch -- where the sparse form saves no more than the full decode's walks above 24: that set keeps the full decode)
    if constexpr (NB > 4) {
        switch (g1) {
            case 4: SELHIP_BS_LAUNCH(4); return;
            case 5: SELHIP_BS_LAUNCH(5); return;
        }
    }
    if constexpr (NB > 5) {
        if (g1 == 6) { SELHIP_BS_LAUNCH(6); return; }
    }
    SELHIP_BS_LAUNCH(0);
#undef SELHIP_BS_LAUNCH
}
// image (with lists, sparse_t <= kBsImageMaxT): the set's clamped image -- the four-plane kernel on its 8 KiB rows, whatever khi is
hipError_t launch_hist_bs(int khi, unsigned blocks, hipStream_t st, const uint32_t* bs, const uint8_t* gmax, const selhip_int2_t* list, const u64* count,
                          u64 cap, uint32_t* counts, u64 off, u64 window, int run, u64 dense_pairs, int sparse_t = 0, const uint32_t* lists = nullptr,
                          const uint32_t* image = nullptr) {
    // (a threshold at or above khi leaves every list empty: there the full decode's per-pair walks already stop below it)
    const int g1 = sparse_t > 0 && sparse_t < khi && lists ? sparse_t / 4 : 0;
    if (image && g1 >= 1 && 4 * g1 <= kBsImageMaxT) {
#define SELHIP_BS_IMAGE(G1) hipLaunchKernelGGL((hll_union_hist_bs_kernel<kBsImagePlanes, G1, kBsImageDwords>), dim3(blocks), dim3(kBlock), 0, st, image, gmax, lists, \
                                               list, count, cap, counts, off, window, run, dense_pairs)
        switch (g1) {
            case 1:  SELHIP_BS_IMAGE(1); break;
            case 2:  SELHIP_BS_IMAGE(2); break;
            default: SELHIP_BS_IMAGE(3);
        }
#undef SELHIP_BS_IMAGE
        return hipGetLastError();
    }
    switch (bs_planes(khi)) {
        case 4:  launch_hist_bs_nb<4>(g1, blocks, st, bs, gmax, lists, list, count, cap, counts, off, window, run, dense_pairs); break;
        case 5:  launch_hist_bs_nb<5>(g1, blocks, st, bs, gmax, lists, list, count, cap, counts, off, window, run, dense_pairs); break;
        default: launch_hist_bs_nb<6>(g1, blocks, st, bs, gmax, lists, list, count, cap, counts, off, window, run, dense_pairs);
    }
    return hipGetLastError();
}

// the sparse lists of n genomes from their planes (kernel_hllbs.cuh); *t = the set's threshold, 0 when it would exceed kBsSparseMaxT
// (nothing written then).  image: the set's clamped image, written by the same kernel where the threshold is at most kBsImageMaxT
// (*image_ok; the threshold is only known here, so the buffer is sized here -- and only ever grown, like every DevBuf: freeing it
// would make the call wait for the whole device).  Waits for the stream.
int build_sparse_lists(std::string* err, hipStream_t st, const uint32_t* d_bs, int64_t n, uint32_t* d_lists, int* d_t, int* t, DevBuf<uint32_t>* image,
                       bool* image_ok) {
    *t = 0;
    *image_ok = false;
    if (n <= 0) return SELHIP_OK;
    HIPCHK(err, hipMemsetAsync(d_t, 0, sizeof(int), st));
    hipLaunchKernelGGL(hll_sparse_t_kernel, dim3(grid_for((u64)n, kWavesPerBlock, 8192)), dim3(kBlock), 0, st, d_bs, (long long)n, d_t);
    HIPCHK(err, hipGetLastError());
    int need = 0;
    HIPCHK(err, hipMemcpyAsync(&need, d_t, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    if (need < 4 || need > kBsSparseMaxT) return SELHIP_OK;
    const bool with_image = need <= kBsImageMaxT;
    if (with_image) HIPCHK(err, image->ensure((size_t)n * kBsImageDwords));
    hipLaunchKernelGGL(hll_sparse_list_kernel, dim3(grid_for((u64)n, kWavesPerBlock, 8192)), dim3(kBlock), 0, st, d_bs, (long long)n, need, d_lists,
                       with_image ? image->p : nullptr);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipStreamSynchronize(st));
    *t = need;
    *image_ok = with_image;
    return SELHIP_OK;
}

bool use_bitslices(const selhip_ctx* c) { return c->p == 14 && c->planes.khi > 0 && c->hist_algo != 0; }
// the set holds a clamped image that stage 2a may read with the lists ("hist_image" != 0; the image exists only for thresholds up to kBsImageMaxT)
bool image_ready(const selhip_ctx* c) { return c->hist_image != 0 && c->hll_image_ok && c->hll_sparse_t >= 4 && c->hll_sparse_t <= kBsImageMaxT; }
// the all-pairs stage 2a's sparse threshold in use (0 = every value from the planes)
// Automatic ("hist_sparse" = -1): where the set's planes fit the Infinity Cache, or the lists come with the clamped image.  Beyond the
// cache the kernel is bound by its fetches of candidate rows, not by instructions, and on the six-plane rows the lists add 512 B to
// each: cfg4 (50 000 genomes, 600 MB of planes) 144.5 -> 146.8 us, its step 1.502 -> 1.515 ms with them (profiles/hist_sparse_ab.txt).
// With the image a candidate row is 8.5 KiB where the full decode reads 10, and the sparse form wins there too: cfg4 1.474 -> 1.422 ms
// a step, cfg5 5.172 -> 5.050 (profiles/hist_image_ab.txt), so the size gate only holds where there is no image (T >= 16, "hist_image" = 0).
constexpr size_t kSparseMaxPlaneBytes = (size_t)192 << 20;
int sparse_t_used(const selhip_ctx* c) {
    if (!use_bitslices(c) || !c->hist_sparse || c->hll_sparse_t >= c->planes.khi) return 0;
    if (c->hist_sparse < 0 && !image_ready(c) && (size_t)c->n * kBsGenomeDwords * sizeof(uint32_t) > kSparseMaxPlaneBytes) return 0;
    if (c->hll_sparse_t > 20 && c->planes.khi <= 32) return 0;                                   // (launch_hist_bs_nb: five planes, G1 = 6)
    return c->hll_sparse_t;
}
// ... and whether it reads the image in place of the six-plane rows: wherever it takes the lists and the image is there.  "hist_image"
// -1 and 1 are the same rule: no size was found at which the shorter rows lose (profiles/hist_image_ab.txt)
bool image_used(const selhip_ctx* c) { return image_ready(c) && sparse_t_used(c) == c->hll_sparse_t; }

int compute_cards(selhip_ctx* c, const uint8_t* d_hll, int64_t n, int p, double* d_out) {
    if (n <= 0) return SELHIP_OK;
    HIPCHK(&c->err, c->self_pairs.ensure((size_t)n));
    HIPCHK(&c->err, c->counts.ensure((size_t)n * 64));
    hipLaunchKernelGGL(iota_pairs_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->self_pairs.p, (int)n);
    HIPCHK(&c->err, hipGetLastError());
    hipLaunchKernelGGL(hll_union_hist_kernel, dim3(grid_for((u64)n, kWavesPerBlock, 4096)), dim3(kBlock), 0, c->stream,
                       d_hll, p, c->self_pairs.p, (const u64*)nullptr, (u64)n, (u64)n, c->counts.p);
    HIPCHK(&c->err, hipGetLastError());
    HIPCHK(&c->err, launch_select<0>(c->fp_mode == SELHIP_FP_FMA, c->stream, grid_for((u64)n, kWave, 8192), c->counts.p,
                                     nullptr, (u64)n, (u64)n, p, d_out, nullptr, nullptr, 0.0, nullptr, 0, nullptr,
                                     nullptr, nullptr));
    return SELHIP_OK;
}

// upper bound of the pair space of rows [rb, re): the triangle (CB can only shrink it)
long long pair_bound(long long n, long long rb, long long re) {
    long long cnt = 0;
    // sum_{i=rb}^{re-1} (n-1-i)
    const long long rows = re - rb;
    cnt = rows * (n - 1) - (rb + re - 1) * rows / 2;
    return cnt < 0 ? 0 : cnt;
}

template <int CRIT>
hipError_t launch_aux_fused(selhip_ctx* c, hipStream_t st, const selhip_int2_t* list, const u64* n_dev, u64 cap, u64 bound, double tau,
                            selhip_int2_t* out, u64 out_cap, u64* out_count) {
    const AuxConsts k = aux_consts(c->p_aux);
    const unsigned grid = grid_for(bound, kWave, 32768);
    with_flag(c->fp_mode == SELHIP_FP_FMA, [&](auto F) {
        hipLaunchKernelGGL((aux_fused_kernel<decltype(F)::value, CRIT>), dim3(grid), dim3(kWave), 0, st, c->d_aux_hll, c->p_aux, list, n_dev, cap,
                           k.rs, c->ecard.p, tau, k.zs, k.S_sum, out, out_cap, out_count);
    });
    return hipGetLastError();
}

// equal-pair row boundaries of the triangle rows [rb, re) x columns (row, n): the same cut the multi-GPU drivers use
// rows after which the deal of the row interleave repeats: two cycles of n_parts blocks (the snake turns round every cycle)
long long interleave_period(const selhip_ctx* c) { return c->il_parts > 1 ? 2ll * c->il_block * c->il_parts : 1; }

void chunk_rows(long long n, long long rb, long long re, int chunks, long long period, long long* bnd) {
    // boundaries fall on whole interleave periods counted from rb (row ownership is defined relative to the range's first row)
    const double total = (double)pair_bound(n, rb, re);
    bnd[0] = rb;
    long long i = rb;
    double acc = 0;
    for (int c = 1; c < chunks; ++c) {
        const double target = total * c / chunks;
        while (i < re && acc < target) {
            const long long e = std::min(re, i + period);
            acc += (double)pair_bound(n, i, e);
            i = e;
        }
        bnd[c] = i;
    }
    bnd[chunks] = re;
}

// the pass joins 16-bit (or 15-bit) signature pairs and verifies what they pass on (launch_stage1_sig's first branch)
bool join16_pass(const selhip_ctx* c) { return c->plan.use_sig && !c->plan.use_hash && c->join_bits <= 16; }

int pipeline_chunks(const selhip_ctx* c) {
    // Round 1's pipeline (stage 1 of every chunk on one stream, stage 2 on another) lost on every configuration and was replaced
    // by whole-chain lanes (enqueue_pass).  Automatic setting: two chunks for the signature join once a pass is large enough for
    // the second set of tail launches to cost less than the overlap wins (measured: profiles/r02_chunk_lanes.txt).
    if (!c->plan.smh || c->pipeline == 0 || c->pipeline == 1 || c->plan.use_hash) return 1;   // (the sort join works on all rows at once)
    if (c->pipeline > 1) return std::min(c->pipeline, kMaxChunks);
    if (!join16_pass(c) || !grouping_on(c)) return 1;
    const double pairs = (double)pair_bound(c->n, c->row_begin, c->row_end) / std::max(1, c->il_parts);
    return pairs >= kAutoChunkPairs ? 2 : 1;
}

// Wait for the context's stream with low wake-up latency: poll for up to ~2 ms (a pass of the BASELINE single-GPU
// configurations takes 0.5-20 ms and the blocking wait's wake-up costs tens of microseconds), then block.
hipError_t wait_stream(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    return hipStreamSynchronize(st);
}

// one chain of a pass: the stream it runs on, the query rows it covers and its slices of the pass's buffers
struct Chain {
    StageIO io;
    int rb, re;
    selhip_int2_t* fin; u64 fin_cap;        // output of the auxiliary criterion
    int* csr_cnt; int* csr_start; char* scan_tmp;
    selhip_int2_t* grouped;
    uint32_t* counts; u64 window;           // histogram scratch: `window` pairs at a time
};

// per-chain row arrays of the grouping: counts | fill cursors | labels | label-group sums (then bucket starts) | roots, n ints each
size_t csr_stride(int n) { return 5 * (size_t)n + 2; }

constexpr double kLabelOrderPairs = 4e8;
constexpr size_t kLabelOrderBytes = (size_t)192 << 20;     // HLL rows beyond this (the Infinity Cache holds 256 MiB): label order
bool label_order(const selhip_ctx* c) {
    if (!grouping_on(c)) return false;
    if (c->group_label >= 0) return c->group_label == 1;
    // the bit-plane kernel is bound by its fetches from beyond L2 at every size (cfg3: stage 2a 79 -> 54 us with the label order)
    if (use_bitslices(c)) return true;
    // its three extra launches (~15 us) only pay where stage 2a is bound by fetches from beyond L2 AND has enough pairs: HLL rows
    // beyond the Infinity Cache and -- the proxy known here -- a large pair space (one of 8 ranks of cfg4, 1.6e8 pairs: 0.515 -> 0.529 ms
    // with it; one of 8 ranks of cfg5, 6.2e8: 1.613 -> 1.577 ms; cfg3, whose rows fit the Infinity Cache: 0.311 -> 0.313 ms)
    return (size_t)c->n * 16384 > kLabelOrderBytes && (double)pair_bound(c->n, c->row_begin, c->row_end) / std::max(1, c->il_parts) >= kLabelOrderPairs;
}

// stage 2 of one chain over a pair list: union histograms, `window` pairs at a time, and the estimator / J test behind each window.
// grouped: the list is bucketed by query row (runs of a row's pairs; a dense list is walked by candidate slice per XCD)
int enqueue_hist_select(selhip_ctx* c, const Chain& ch, const selhip_int2_t* final_list, const u64* final_count, u64 final_cap,
                        bool grouped, double tau, PassCounters* pc0) {
    hipStream_t st = ch.io.st;
    for (u64 off = 0; off < final_cap; off += ch.window) {
        {
            TimerScope t(c, T_HIST, st);
            if (use_bitslices(c)) c->hist_image_used = image_used(c) ? 1 : 0;
            if (use_bitslices(c))
                HIPCHK(&c->err, launch_hist_bs(c->planes.khi, (unsigned)c->hist_bs_blocks, st, c->planes.bs.p, c->planes.gmax.p, final_list, final_count, final_cap, ch.counts, off, ch.window,
                                               c->hist_run > 0 ? c->hist_run : (grouped ? 4 : 1),
                                               // a dense survivor graph is walked by candidate-row slice per XCD (query-major list only)
                                               // ("dense" = survivors per QUERY ROW of this chain: a rank's or a lane's share of the rows sees
                                               //  its share of the pairs and all of the candidate rows)
                                               grouped && c->hist_dense_degree >= 0
                                                   ? (u64)c->hist_dense_degree * (u64)std::max<long long>(1, ((long long)ch.re - ch.rb) / std::max(1, c->il_parts)) : ~0ull,
                                               sparse_t_used(c), c->hll_sparse.p, image_used(c) ? c->hll_image.p : nullptr));
            else if (c->p == 14)
                hipLaunchKernelGGL(hll_union_hist_runs_kernel, dim3(c->hist_blocks), dim3(kWave), (size_t)c->hist_pad, st,
                                   c->d_hll, final_list, final_count, final_cap, ch.counts, off, ch.window,
                                   c->hist_run > 0 ? c->hist_run : (grouped && label_order(c) ? 4 : 1));
            else
                hipLaunchKernelGGL(hll_union_hist_kernel, dim3(2048), dim3(kBlock), 0, st,
                                   c->d_hll, c->p, final_list, final_count, (u64)0, final_cap, ch.counts, off, ch.window);
            HIPCHK(&c->err, hipGetLastError());
        }
        TimerScope t(c, T_SELECT, st);
        HIPCHK(&c->err, launch_select<1>(c->fp_mode == SELHIP_FP_FMA, st, 4096, ch.counts, final_count, 0,
                                         final_cap, c->p, nullptr, final_list, c->ecard.p, tau,
                                         c->results.p, (u64)c->results.cap, pc0, nullptr, nullptr, off, ch.window, c->measure));
    }
    return SELHIP_OK;
}

int enqueue_tail(selhip_ctx* c, const Chain& ch, const selhip_int2_t* final_list, const u64* final_count, u64 final_cap,
                 bool counted, double tau, PassCounters* pc0) {
    const int n = (int)c->n;
    hipStream_t st = ch.io.st;
    const bool grouped = grouping_on(c);
    if (grouped) {
        // bucket the final list by query row so that stage 2a can keep that row in registers across its pairs
        TimerScope t(c, T_GROUP, st);
        // (the counters were cleared by the pass's first kernel)
        const bool label = label_order(c);
        int* const cnt = ch.csr_cnt; int* const fill = cnt + n; int* const lab = cnt + 2 * (size_t)n; int* const gsum = cnt + 3 * (size_t)n;
        if (!counted) {
            hipLaunchKernelGGL(csr_count_kernel, dim3(512), dim3(kBlock), 0, st, final_list, final_count, final_cap, cnt, label ? lab : nullptr, n);
            HIPCHK(&c->err, hipGetLastError());
        }
        if (label && n <= kSmallScanMax) {
            int* const root = cnt + 4 * (size_t)n;
            hipLaunchKernelGGL(csr_label_offsets_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, st, cnt, lab, n, gsum, root, ch.csr_start);
            HIPCHK(&c->err, hipGetLastError());
            if ((size_t)n * sizeof(int) > 48 * 1024)
                HIPCHK(&c->err, hipFuncSetAttribute((const void*)csr_label_scan_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmallScanMax * 4));
            hipLaunchKernelGGL(csr_label_scan_fill_kernel, dim3(256), dim3(1024), (size_t)n * sizeof(int), st, gsum, n, root, ch.csr_start,
                               final_list, final_count, final_cap, fill, ch.grouped);
            HIPCHK(&c->err, hipGetLastError());
        } else if (label) {
            const unsigned row_blocks = (unsigned)((n + kBlock - 1) / kBlock);
            hipLaunchKernelGGL(csr_label_sum_kernel, dim3(row_blocks), dim3(kBlock), 0, st, cnt, lab, n, gsum);
            HIPCHK(&c->err, hipGetLastError());
            size_t tmp_bytes = c->scan_tmp_stride;
            HIPCHK(&c->err, rocprim::exclusive_scan(ch.scan_tmp, tmp_bytes, gsum, ch.csr_start, 0, (size_t)n, rocprim::plus<int>(), st));
            hipLaunchKernelGGL(csr_label_assign_kernel, dim3(row_blocks), dim3(kBlock), 0, st, cnt, lab, n, ch.csr_start, gsum);   // gsum := bucket starts
            HIPCHK(&c->err, hipGetLastError());
            hipLaunchKernelGGL(csr_fill_kernel, dim3(512), dim3(kBlock), 0, st, final_list, final_count, final_cap, gsum, fill, ch.grouped);
            HIPCHK(&c->err, hipGetLastError());
        } else if (n <= kSmallScanMax) {
            if ((size_t)n * sizeof(int) > 48 * 1024)       // per device, so not cached in a process-wide flag (selhip_multi_select drives several)
                HIPCHK(&c->err, hipFuncSetAttribute((const void*)csr_scan_fill_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, kSmallScanMax * 4));
            hipLaunchKernelGGL(csr_scan_fill_kernel, dim3(256), dim3(1024), (size_t)n * sizeof(int), st, cnt, n,
                               final_list, final_count, final_cap, fill, ch.grouped);
            HIPCHK(&c->err, hipGetLastError());
        } else {
            size_t tmp_bytes = c->scan_tmp_stride;
            HIPCHK(&c->err, rocprim::exclusive_scan(ch.scan_tmp, tmp_bytes, cnt, ch.csr_start, 0, (size_t)n, rocprim::plus<int>(), st));
            hipLaunchKernelGGL(csr_fill_kernel, dim3(512), dim3(kBlock), 0, st, final_list, final_count, final_cap,
                               ch.csr_start, fill, ch.grouped);
            HIPCHK(&c->err, hipGetLastError());
        }
        final_list = ch.grouped;
    }
    return enqueue_hist_select(c, ch, final_list, final_count, final_cap, grouped, tau, pc0);
}

// smh_a (alone or before the auxiliary criterion) or the count of smh_c over the query rows of one chain, then the final criterion.  [rb, re) is the
// pass's whole row range (row ownership under the interleave is counted from its first row)
int enqueue_chain(selhip_ctx* c, const Chain& ch, int rb, int re, double tau, bool use_hash, bool use_sig, bool count_in_verify,
                  PassCounters* pc0) {
    const StageIO& io = ch.io;
    RowMap rm = row_map(c, rb, re);
    if (c->il_parts <= 1) rm = row_map(c, ch.rb, ch.re);
    else { rm.row_begin = ch.rb; rm.row_end = ch.re; }          // ch.rb - rb is a multiple of the interleave period
    {
        TimerScope t(c, T_STAGE1, io.st);
        if (c->plan.count) HIPCHK(&c->err, launch_stage1_count(c, io, rm));
        else if (use_hash) HIPCHK(&c->err, launch_stage1_hashjoin(c, io, c->n_rows, c->n_bands, rm));
        else if (use_sig) HIPCHK(&c->err, launch_stage1_sig(c, io, c->n_rows, c->n_bands, rm));
        else              HIPCHK(&c->err, launch_stage1(c, io, c->n_rows, c->n_bands, rm));
    }
    if (c->plan.emit) return SELHIP_OK;                          // the count kernel wrote the records: nothing is left for a stage 2
    const selhip_int2_t* final_list = io.surv;
    const u64* final_count = &io.pc->n_survivors;
    u64 final_cap = io.cap;
    if (c->criterion == SELHIP_CRIT_HLL_A_SMH_A) {
        // two-stage form (BASELINE configs[4]): the auxiliary criterion (histogram + estimator + test fused, one lane per pair)
        // sees the survivors of the smh_a join
        TimerScope t(c, T_AUX, io.st);
        HIPCHK(&c->err, launch_aux_fused<1>(c, io.st, io.surv, &io.pc->n_survivors, io.cap, io.cap, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
        final_list = ch.fin;
        final_count = &io.pc->n_final;
        final_cap = ch.fin_cap;
    }
    return enqueue_tail(c, ch, final_list, final_count, final_cap, count_in_verify, tau, pc0);
}

// ---- the whole pass of a small set in one cooperative launch (kernel_small.cuh) ------------------------------------------------
bool small_pass_ok(const selhip_ctx* c) {
    if (c->small_pass == 0 || c->small_pass_failed) return false;
    if (c->n < 2 || c->n > kSmallPassMaxN || c->criterion != SELHIP_CRIT_SMH_A || c->il_parts > 1) return false;
    if (c->measure != SELHIP_MEASURE_JACCARD) return false;                  // (the kernel's stage 2 is the J test alone)
    if (!c->plan.use_sig || c->plan.use_hash) return false;
    if (!sig_tile_shape(c->m, c->n_rows, c->n_bands)) return false;          // the kernel always builds in tiles, whatever "sig_tile" says
    if ((c->row_end - c->row_begin + 255) / 256 > kSmallRows) return false;                        // rows per block of the 256-block grid
    if (c->dev_cus < 256) return false;                                                            // (a partitioned or masked device: the regular pass)
    return use_bitslices(c) && c->planes.khi <= 32;                                                   // bit planes, at most five of them non-zero
}

template <bool FMA, int NB>
hipError_t launch_small_pass(selhip_ctx* c, PassCounters* pc_next, double tau) {
    int n = (int)c->n;
    int n_pad = pad_wave(n);
    RowMap rm = row_map(c, (int)c->row_begin, (int)c->row_end);
    int m = c->m, r = c->n_rows, nb = c->n_bands, use_cb = c->mode == SELHIP_MODE_CB_SMH ? 1 : 0, cand_begin = (int)c->cand_begin, fb = c->verify_fb;
    const u64* aux = c->d_aux; const double* cards = c->d_cards; const uint32_t* bs = c->planes.bs.p; const uint8_t* gmax = c->planes.gmax.p;
    uint32_t *sQ = c->sig.Q.p, *sT = c->sig.T.p, *sP = c->sig.P.p, *sG = c->sig.G.p;
    u64* ecard = c->ecard.p; int* hi = c->hi.p; PassCounters* pc = c->pcb;
    u64* barrier_word = &c->pcb[kMaxChunks].n_aux_in;                   // a word of this pass's counter set that nothing else uses (cleared by the previous pass)
    if (!c->small_bar.p) {                                               // the barrier's group words: zero between passes (the kernel puts them back)
        hipError_t e = c->small_bar.ensure((size_t)kSmallBarGroups * kSmallBarStride);
        if (e == hipSuccess) e = hipMemsetAsync(c->small_bar.p, 0, sizeof(u64) * kSmallBarGroups * kSmallBarStride, c->stream);
        if (e != hipSuccess) return e;
    }
    u64* barrier_groups = c->small_bar.p;
    u64 barrier_ticks = c->small_pass == 3 ? 0 : 2000000;                // 20 ms of the 100 MHz wall clock ("small_pass" = 3, test hook: no wait at all)
    double rs = relerr_scaled_for(14);
    selhip_pair_t* results = c->results.p; u64 results_cap = (u64)c->results.cap;
    void* args[] = {&aux, &cards, &bs, &gmax, &n, &m, &r, &nb, &n_pad, &tau, &use_cb, &rm, &cand_begin, &sQ, &sT, &sP, &sG, &ecard, &hi, &pc, &pc_next,
                    &barrier_word, &barrier_groups, &barrier_ticks, &rs, &results, &results_cap, &fb};
    const unsigned grid = 256;                                           // one block per CU (small_pass_ok checked that the device has 256)
    // an ordinary launch: 256 blocks of 256 threads with 60 KB of LDS and <= 250 registers -- a CU holds two, the device 512 -- all become
    // resident as soon as whatever else is running drains, which is all the kernel's one barrier needs (work of the same stream is over
    // by then; nothing another stream runs waits for this kernel); hipLaunchCooperativeKernel ("small_pass" = 2) asks the runtime for
    // that guarantee and costs ~15 us more per launch
    if (c->small_pass == 2) return hipLaunchCooperativeKernel((const void*)small_pass_kernel<FMA, NB>, dim3(grid), dim3(kBlock), args, 0, c->stream);
    return hipLaunchKernel((const void*)small_pass_kernel<FMA, NB>, dim3(grid), dim3(kBlock), args, 0, c->stream);
}

int enqueue_small_pass(selhip_ctx* c, PassCounters* pc_next, double tau) {
    TimerScope t(c, T_STAGE1);
    c->sig_key = 0;                                                      // (the kernel rewrites the 32-bit signature layouts only)
    const hipError_t e = with_flag(c->fp_mode == SELHIP_FP_FMA, [&](auto F) {
        return bs_planes(c->planes.khi) == 4 ? launch_small_pass<decltype(F)::value, 4>(c, pc_next, tau) : launch_small_pass<decltype(F)::value, 5>(c, pc_next, tau);
    });
    HIPCHK(&c->err, e);
    return SELHIP_OK;
}

// ---- criterion "none" (kernel_dense.cuh) ---------------------------------------------------------------------------------------
// what SELHIP_CRIT_NONE asks of the context: p = 14 sketches with their bit planes resident (there is no byte-row form of the pass).
// An accepted pass has its route from here on ("dense_route_used"), also one that turns out empty and launches nothing
int accept_dense(selhip_ctx* c) {
    if (c->p != 14 || (c->n > 0 && !use_bitslices(c))) {
        set_err(&c->err, "criterion none (SELHIP_CRIT_NONE) needs p_hll = 14 sketches and their bit planes (p_hll = %d, hist_algo = %d)", c->p, c->hist_algo);
        return SELHIP_E_BADARG;
    }
    c->dense_route_used = c->dense_fused ? 1 : 0;
    return SELHIP_OK;
}

// the empty criterion passes every evaluated pair on: survivors = candidates = evaluated
void dense_stats(PassCounters* pc) { pc->n_survivors = pc->n_final = pc->n_candidates = pc->n_evaluated; }

// dense_select_kernel over the rows of rm against the candidates from first_cand on.  lo == nullptr: an all-pairs pass (X = Y, ranges
// from hi and pc_in's z0), else a query pass (windows lo / hi).  khi = largest register value + 1 of the two sets
hipError_t launch_dense(bool fma, hipStream_t st, int khi, const DenseSet& X, const DenseSet& Y, int n_y, const int* lo, const int* hi,
                        const PassCounters* pc_in, const RowMap& rm, int first_cand, double tau, selhip_pair_t* results, u64 results_cap,
                        PassCounters* pc, int measure) {
    const long long n_tiles = rm.n_tiles(kWavesPerBlock);
    const int span_base = first_cand / kDenseSpan;
    const long long n_spans = ((long long)n_y + kDenseSpan - 1) / kDenseSpan - span_base;
    if (n_tiles <= 0 || n_spans <= 0) return hipSuccess;
    if (n_tiles > 0x7FFFFFFFll) return hipErrorInvalidValue;
    const long long n_units = 8 * n_tiles * ((n_spans + 7) / 8);
    const unsigned grid = (unsigned)std::min<long long>(n_units, 0x7FFFFFF8ll);              // (a multiple of 8; beyond it blocks take several units)
    const double rs = relerr_scaled_for(14);
    with_flag(fma, [&](auto F) { with_flag(measure == SELHIP_MEASURE_MAX_CONTAINMENT, [&](auto C) {
        constexpr int MEAS = decltype(C)::value ? SELHIP_MEASURE_MAX_CONTAINMENT : SELHIP_MEASURE_JACCARD;
#define SELHIP_DENSE_LAUNCH(NB) hipLaunchKernelGGL((dense_select_kernel<NB, decltype(F)::value, MEAS>), dim3(grid), dim3(kBlock), 0, st, X, Y, n_y, lo, hi, pc_in, rm, \
                                                   (int)n_tiles, span_base, n_units, tau, rs, results, results_cap, pc)
        switch (bs_planes(khi)) {
            case 4:  SELHIP_DENSE_LAUNCH(4); break;
            case 5:  SELHIP_DENSE_LAUNCH(5); break;
            default: SELHIP_DENSE_LAUNCH(6);
        }
#undef SELHIP_DENSE_LAUNCH
    }); });
    return hipGetLastError();
}

// the all-pairs pass of SELHIP_CRIT_NONE in one launch behind cb_bounds_kernel
int enqueue_dense(selhip_ctx* c, int rb, int re, double tau, PassCounters* pc0) {
    TimerScope t(c, T_DENSE);
    const DenseSet set{c->planes.bs.p, c->planes.gmax.p, c->ecard.p};
    HIPCHK(&c->err, launch_dense(c->fp_mode == SELHIP_FP_FMA, c->stream, c->planes.khi, set, set, (int)c->n, nullptr, c->hi.p, pc0, row_map(c, rb, re),
                                 std::max(rb + 1, (int)c->cand_begin), tau, c->results.p, (u64)c->results.cap, pc0, c->measure));
    return SELHIP_OK;
}

// chunk k's slices of the pass's buffers (one chunk = the whole of each); pc0 = the pass's counter block 0
Chain chain_slices(selhip_ctx* c, int k, int chunks, hipStream_t st, long long b, long long e, PassCounters* pc0, bool count_in_verify) {
    const int n = (int)c->n;
    const u64 slice = (u64)c->surv.cap / (u64)chunks;
    Chain ch;
    ch.io = StageIO{st, c->cand.p + (size_t)k * slice, c->surv.p + (size_t)k * slice, slice, pc0 + 1 + k};
    ch.io.seg_cnt = c->seg_cnt.p + (size_t)(1 + k) * kAppendSegs * kSegStride;
    ch.rb = (int)b; ch.re = (int)e;
    ch.fin = c->fin.p ? c->fin.p + (size_t)k * ((u64)c->fin.cap / (u64)chunks) : nullptr;
    ch.fin_cap = (u64)c->fin.cap / (u64)chunks;
    ch.csr_cnt = c->csr_cnt.p ? c->csr_cnt.p + (size_t)k * csr_stride(n) : nullptr;
    ch.csr_start = c->csr_start.p ? c->csr_start.p + (size_t)k * ((size_t)n + 2) : nullptr;
    ch.scan_tmp = c->scan_tmp.p ? c->scan_tmp.p + (size_t)k * c->scan_tmp_stride : nullptr;
    ch.grouped = c->grouped.p ? c->grouped.p + (size_t)k * slice : nullptr;
    ch.window = ((u64)c->counts.cap / 64) / (u64)chunks;
    ch.counts = c->counts.p + (size_t)k * ch.window * 64;
    if (count_in_verify) { ch.io.row_cnt = ch.csr_cnt; if (label_order(c)) ch.io.row_lab = ch.csr_cnt + 2 * (size_t)n; }
    return ch;
}

int enqueue_pass(selhip_ctx* c) {
    const int n = (int)c->n;
    // (a pass in row rounds, selhip_ctx_set_topk_rounds: the rows of the round in hand -- a sub-range pass -- instead of the pass's)
    const int rb = (int)(c->rd.on ? c->rd.begin : c->row_begin), re = (int)(c->rd.on ? c->rd.end : c->row_end);
    const double tau = (double)c->tau_f;            // float threshold widened, selection.cpp:81,164
    const int crit = c->criterion;
    const PassPlan& plan = c->plan;
    c->dominant_timer = c->timed_kernel == 1 ? T_HIST : crit == SELHIP_CRIT_NONE ? T_DENSE : (plan.use_sig ? T_JOIN : T_STAGE1);
    if (c->timing && !(c->rd.on && c->rd.begin != c->row_begin)) c->timed_passes += 1;       // (the rounds of a pass are one pass)
    TimerScope total(c, T_TOTAL);
    const bool smh_crit = plan.smh, use_hash = plan.use_hash, use_sig = plan.use_sig;
    if (plan.bad) { set_err(&c->err, plan.bad, c->n_rows, c->n_bands); return SELHIP_E_BADARG; }
    // counter set of this pass (block 0: z0, evaluated, results; blocks 1.. : one per row chunk); the other set is cleared by
    // this pass's first kernel for the next pass.  (Claimed only now: nothing above launches, and an argument error must not consume
    // a set that no kernel has cleared.)  It stays dirty until this function returns SELHIP_OK
    CounterSets::Claim pcs;
    HIPCHK(&c->err, c->pc.claim(c->stream, &pcs));
    c->pcb = pcs.cur;
    PassCounters* const pc_next = pcs.next;
    PassCounters* pc0 = c->pcb;
    if (c->fail_after_flip) { c->fail_after_flip = 0; set_err(&c->err, "test hook: enqueue failed after the counter flip"); return SELHIP_E_HIP; }
    c->small_used = small_pass_ok(c);
    c->hist_image_used = 0;                         // (enqueue_hist_select says otherwise)
    if (c->small_used) {
        c->n_chunks_last = 1;
        const int rc = enqueue_small_pass(c, pc_next, tau);
        if (rc) return rc;
        HIPCHK(&c->err, hipMemcpyAsync(c->h_pc, c->pcb, sizeof(PassCounters) * (kMaxChunks + 1), hipMemcpyDeviceToHost, c->stream));
        c->pc.dirty = false;
        return SELHIP_OK;
    }
    if (use_sig) {
        // bounds (truncated cards, CB cut-offs, z0, evaluated count) ride in the first blocks of the signature build
        HIPCHK(&c->err, launch_sig_build(c, c->n_rows, c->n_bands, tau, rb, re, pc_next));
    } else {
        TimerScope t(c, T_PREP);
        hipLaunchKernelGGL(cb_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_cards, n, tau, c->mode == SELHIP_MODE_CB_SMH ? 1 : 0, row_map(c, rb, re), c->ecard.p, c->hi.p, pc0,
                           grouping_on(c) && !plan.emit ? c->csr_cnt.p : nullptr, grouping_on(c) && !plan.emit ? (int)c->csr_cnt.cap : 0, (int)c->cand_begin, pc_next,
                           c->seg_cnt.p, (int)c->seg_cnt.cap);
        HIPCHK(&c->err, hipGetLastError());
        if (plan.il_stream) {
            // ALGO_STREAM: the bucket-interleaved copy of the sketches (lane l = buckets [l*B, (l+1)*B)), rebuilt every pass
            const int nch = c->m / 128;
            const long long total = (long long)c->n * nch * kWave;
            hipLaunchKernelGGL(stream_interleave_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                               reinterpret_cast<const u64x2*>(c->d_aux), reinterpret_cast<u64x2*>(c->aux_il.p), total, nch);
            HIPCHK(&c->err, hipGetLastError());
        }
    }

    const int chunks = pipeline_chunks(c);
    c->n_chunks_last = chunks;
    const bool count_in_verify = crit == SELHIP_CRIT_SMH_A && join16_pass(c) && grouping_on(c);
    auto chain_of = [&](int k, hipStream_t st, long long b, long long e) { return chain_slices(c, k, chunks, st, b, e, pc0, count_in_verify); };
    if (chunks > 1) {
        // ---- row chunks, each a whole chain (join -> verify -> [auxiliary criterion] -> grouping -> histogram -> estimate) on one of
        // two streams: while one chunk's short tail kernels (tens of microseconds each, far too few waves to fill the chip) run, the
        // other chunk's join has the vector units, and the join's own ramp and tail overlap with the neighbour.  Measured with two
        // contexts on two streams before it was built (scripts/overlap_probe.py): cfg4 on one of 8 ranks 0.551 -> 0.544 ms even with
        // the signature build done twice.
        long long bnd[kMaxChunks + 1];
        chunk_rows(n, rb, re, chunks, interleave_period(c), bnd);
        // lane 0 is the context's own stream (cross-stream waits cost ~10 us each: one to start lane 1, one to join it).
        // (Staggering the lanes -- chunk k's join waits for chunk k-1's join, so that every tail runs beside the NEXT join and only the
        // last tail is exposed -- was measured: cfg4 2.78 vs 2.73 ms, cfg5 9.79 vs 9.74 ms with 2 chunks, no better with 4: the tail
        // kernels take from the join what they use, the chip is not idle in either phase.  profiles/r02_chunk_lanes.txt)
        hipStream_t lane[2] = {c->stream, c->st_stage1};
        HIPCHK(&c->err, hipEventRecord(c->ev_start, c->stream));
        HIPCHK(&c->err, hipStreamWaitEvent(lane[1], c->ev_start, 0));
        for (int k = 0; k < chunks; ++k) {
            // odd chunks first in program order so that lane 1's work is queued before lane 0's blocks the host thread's view
            const Chain ch = chain_of(k, lane[(k & 1) ^ 1], bnd[k], bnd[k + 1]);
            const int rc = enqueue_chain(c, ch, rb, re, tau, use_hash, use_sig, count_in_verify, pc0);
            if (rc) return rc;
        }
        HIPCHK(&c->err, hipEventRecord(c->ev_end, lane[1]));
        HIPCHK(&c->err, hipStreamWaitEvent(c->stream, c->ev_end, 0));
        HIPCHK(&c->err, hipMemcpyAsync(c->h_pc, c->pcb, sizeof(PassCounters) * (kMaxChunks + 1), hipMemcpyDeviceToHost, c->stream));
        c->pc.dirty = false;
        return SELHIP_OK;
    }

    // ---- single chunk: everything in order on the context's stream (counter block 1)
    const Chain ch = chain_of(0, c->stream, rb, re);
    if (smh_crit) {
        const int rc = enqueue_chain(c, ch, rb, re, tau, use_hash, use_sig, count_in_verify, pc0);
        if (rc) return rc;
    } else if (crit == SELHIP_CRIT_NONE && c->dense_fused) {
        const int rc = enqueue_dense(c, rb, re, tau, pc0);
        if (rc) return rc;
    } else {
        // hll_a / hll_an as FIRST criterion (selection.cpp:152-173, 206-227): the (CB-pruned) pair space of the rows is listed
        // explicitly, kEnumPairs pairs at a time -- row sub-ranges in turn on the stream, each listed into the same buffer and
        // filtered into `fin` before the next one overwrites it (the reference has no limit on N here; round 1 refused
        // more than 2^28 pairs per call).  Sub-range boundaries fall on whole interleave periods so that row ownership
        // (RowMap blocks are counted from the range's first row) is the same as for the whole range.
        const StageIO& io = ch.io;
        const long long period = interleave_period(c);
        long long sb = rb;
        while (sb < re) {
            long long se = sb;
            long long acc = 0;
            while (se < re) {
                const long long step_end = std::min<long long>(re, se + period);
                const long long add = pair_bound(n, se, step_end);
                if (se > sb && acc + add > c->enum_pairs) break;
                acc += add; se = step_end;
            }
            if ((u64)acc + 1024 > (u64)c->cand.cap) { set_err(&c->err, "internal: enumeration buffer too small for rows [%lld,%lld)", sb, se); return SELHIP_E_OVERFLOW; }
            {
                TimerScope t(c, T_STAGE1);
                HIPCHK(&c->err, hipMemsetAsync(&io.pc->n_aux_in, 0, sizeof(u64), c->stream));
                RowMap rm = row_map(c, rb, re);
                if (c->il_parts <= 1) { rm = row_map(c, (int)sb, (int)se); }
                else { rm.row_begin = (int)sb; rm.row_end = (int)se; }            // sb - rb is a multiple of the interleave period
                const long long rows = rm.n_tiles(1);
                const long long blocks = rows * ((n + kEnumSpan - 1) / kEnumSpan);
                if (blocks > 0x7FFFFFFFll) { set_err(&c->err, "row range too large"); return SELHIP_E_BADARG; }
                if (blocks > 0) {
                    hipLaunchKernelGGL(enum_pairs_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, n, c->hi.p, pc0,
                                       rm, (int)rows, c->cand.p, (u64)c->cand.cap, io.pc);
                    HIPCHK(&c->err, hipGetLastError());
                }
            }
            const u64 bound = std::min<u64>((u64)c->cand.cap, (u64)acc);
            if (crit == SELHIP_CRIT_NONE) {
                // the list route of criterion none: nothing filters the sub-pass's list, stage 2 takes all of it (a row's pairs are
                // neighbours in it, like in a grouped list) before the next sub-pass overwrites it
                const int rc = enqueue_hist_select(c, ch, c->cand.p, &io.pc->n_aux_in, bound, true, tau, pc0);
                if (rc) return rc;
                sb = se;
                continue;
            }
            TimerScope t(c, T_AUX);
            if (crit == SELHIP_CRIT_HLL_AN) HIPCHK(&c->err, launch_aux_fused<2>(c, c->stream, c->cand.p, &io.pc->n_aux_in, (u64)c->cand.cap, bound, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
            else                            HIPCHK(&c->err, launch_aux_fused<1>(c, c->stream, c->cand.p, &io.pc->n_aux_in, (u64)c->cand.cap, bound, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
            sb = se;
        }
        if (crit != SELHIP_CRIT_NONE) {
            const int rc = enqueue_tail(c, ch, ch.fin, &io.pc->n_final, ch.fin_cap, false, tau, pc0);
            if (rc) return rc;
        }
    }
    // (handing the counters to the host from the last block of the final kernel instead of this copy was tried: the 1 024
    // "block done" atomics on one address cost 16 us, the copy dispatch 4)
    HIPCHK(&c->err, hipMemcpyAsync(c->h_pc, c->pcb, sizeof(PassCounters) * (kMaxChunks + 1), hipMemcpyDeviceToHost, c->stream));
    c->pc.dirty = false;
    return SELHIP_OK;
}

int ensure_scratch(selhip_ctx* c, size_t surv_cap, size_t res_cap) {
    HIPCHK(&c->err, c->ecard.ensure((size_t)c->n));
    HIPCHK(&c->err, c->hi.ensure((size_t)c->n));
    if (!c->pc.buf.p) {
        HIPCHK(&c->err, c->pc.buf.ensure(2 * (kMaxChunks + 1)));
        HIPCHK(&c->err, hipMemsetAsync(c->pc.buf.p, 0, sizeof(PassCounters) * 2 * (kMaxChunks + 1), c->stream));
        c->pc.flip = 0;
    }
    HIPCHK(&c->err, c->seg_cnt.ensure(kSegCounterSlots));
    if (!c->st_stage1) {
        HIPCHK(&c->err, hipStreamCreateWithFlags(&c->st_stage1, hipStreamNonBlocking));
        HIPCHK(&c->err, hipEventCreateWithFlags(&c->ev_start, hipEventDisableTiming));
        HIPCHK(&c->err, hipEventCreateWithFlags(&c->ev_end, hipEventDisableTiming));
    }
    HIPCHK(&c->err, c->surv.ensure(surv_cap));
    HIPCHK(&c->err, c->cand.ensure(surv_cap));
    if (aux_criterion(c->criterion)) HIPCHK(&c->err, c->fin.ensure(surv_cap));
    const bool dense_list = c->criterion == SELHIP_CRIT_NONE && !c->dense_fused;       // the list route: the pair space is listed like hll_a's
    if (c->criterion == SELHIP_CRIT_HLL_A || c->criterion == SELHIP_CRIT_HLL_AN || dense_list) {
        // the explicit pair space is materialised kEnumPairs pairs at a time (8 B per pair); one interleave period of rows is the
        // smallest unit, so the buffer holds at least that
        const long long period = interleave_period(c);
        long long unit = 0;
        for (long long s = c->row_begin; s < c->row_end; s += period) unit = std::max(unit, pair_bound(c->n, s, std::min<long long>(c->row_end, s + period)));
        const long long bound = std::min(pair_bound(c->n, c->row_begin, c->row_end), std::max(c->enum_pairs, unit));
        HIPCHK(&c->err, c->cand.ensure((size_t)bound + 1024));
    }
    {
        const size_t nb = (size_t)std::max(c->n_bands, 1);
        const bool hash = c->algo == SELHIP_ALGO_HASHJOIN;
        if (c->plan.il_stream) HIPCHK(&c->err, c->aux_il.ensure((size_t)c->n * c->m));
        if (nb <= 128 || hash) {
            bool moved = false;
            const hipError_t e = c->sig.ensure((size_t)c->n, nb, &moved);
            if (moved) c->sig_key = 0;                                      // the cached signatures went with the arrays
            HIPCHK(&c->err, e);
        }
        if (hash) {
            const size_t total = (size_t)c->n * nb;
            HIPCHK(&c->err, c->hj_keys_in.ensure(total)); HIPCHK(&c->err, c->hj_keys_out.ensure(total));
            HIPCHK(&c->err, c->hj_vals_in.ensure(total)); HIPCHK(&c->err, c->hj_vals_out.ensure(total));
            size_t tmp_bytes = 0;
            HIPCHK(&c->err, rocprim::radix_sort_pairs(nullptr, tmp_bytes, c->hj_keys_in.p, c->hj_keys_out.p, c->hj_vals_in.p,
                                                      c->hj_vals_out.p, total, 0u, 64u, c->stream));
            HIPCHK(&c->err, c->hj_tmp.ensure(tmp_bytes + 256));
        }
    }
    // histogram scratch: 256 B per pair, at most 4 Mi pairs per window (1 GiB of 288; the lists are sized for the join's 16-bit
    // matches, several times the final list, so a smaller window only adds empty histogram + estimate launches: 6 -> 2 per chain at cfg5)
    // (the list route of criterion none puts whole sub-passes through it: the full window)
    HIPCHK(&c->err, c->counts.ensure(std::min<size_t>(std::max(dense_list ? c->cand.cap : c->surv.cap, (size_t)c->n), (size_t)1 << 22) * 64));
    HIPCHK(&c->err, c->results.ensure(res_cap));
    if (grouping_on(c)) {
        const size_t chunks = (size_t)pipeline_chunks(c);               // every chunk lane has its own row counters and scan scratch
        HIPCHK(&c->err, c->csr_cnt.ensure(chunks * csr_stride((int)c->n)));
        HIPCHK(&c->err, c->csr_start.ensure(chunks * ((size_t)c->n + 2)));
        HIPCHK(&c->err, c->grouped.ensure(surv_cap));
        size_t tmp_bytes = 0;
        HIPCHK(&c->err, rocprim::exclusive_scan(nullptr, tmp_bytes, c->csr_cnt.p, c->csr_start.p, 0, (size_t)c->n, rocprim::plus<int>(), c->stream));
        c->scan_tmp_stride = std::max(c->scan_tmp_stride, (tmp_bytes + 511) / 256 * 256);
        HIPCHK(&c->err, c->scan_tmp.ensure(chunks * c->scan_tmp_stride));
    }
    if (!c->h_pc) HIPCHK(&c->err, hipHostMalloc((void**)&c->h_pc, sizeof(PassCounters) * (kMaxChunks + 1), hipHostMallocDefault));
    return SELHIP_OK;
}

}  // namespace

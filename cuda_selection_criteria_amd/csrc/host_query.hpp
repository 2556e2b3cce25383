// host_query.hpp -- the query pass of libselhip.so: a query set Q against the context's database D (kernel_query.cuh), with the
// overflow / repeat and timing bookkeeping of the all-pairs pass.  It has buffers and counters of its own (selhip_ctx::q): only the
// result list and the statistics of the last run are shared with the all-pairs pass.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_pass.hpp); not a stand-alone header.
#pragma once

namespace {

void drop_queries(selhip_ctx* c) {
    c->q.n = -1;
    c->q.d_aux_hll = nullptr; c->q.p_aux = 0;
    c->q.db_sig_key = 0;
    c->q.db_sig_builds = 0;
    c->q.db_idx_key = 0;
    c->q.db_idx_builds = 0;
    c->db_gen += 1;
}

void release_queries(selhip_ctx* c) {
    auto& q = c->q;
    q.own_hll.release(); q.own_aux.release(); q.own_cards.release(); q.planes.release();
    q.lo.release(); q.hi.release(); q.ecard.release();
    q.sig.release(); q.db_sig.release(); q.db_planes.release();
    q.db_idx_sig.release(); q.db_idx_rank.release(); q.db_idx_dir.release();
    q.cand.release(); q.surv.release(); q.fin.release(); q.own_aux_hll.release(); q.counts.release(); q.pc.buf.release();
    if (q.h_pc) (void)hipHostFree(q.h_pc);
    q.h_pc = nullptr;
}

// stage 2a of a query pass on the bit planes of the two sets
hipError_t launch_query_hist(hipStream_t st, const BitPlanes& pq, const BitPlanes& pd, int n_q, const selhip_int2_t* list, const u64* count, u64 cap,
                             uint32_t* counts, u64 off, u64 window) {
    const unsigned blocks = grid_for(std::min<u64>(cap, window), kWavesPerBlock, 4096);
#define SELHIP_QH_LAUNCH(NB) hipLaunchKernelGGL((query_union_hist_kernel<NB>), dim3(blocks), dim3(kBlock), 0, st, pq.bs.p, pq.gmax.p, pd.bs.p, pd.gmax.p, n_q, \
                                                list, count, cap, counts, off, window)
    switch (bs_planes(std::max(pq.khi, pd.khi))) {
        case 4:  SELHIP_QH_LAUNCH(4); break;
        case 5:  SELHIP_QH_LAUNCH(5); break;
        default: SELHIP_QH_LAUNCH(6);
    }
#undef SELHIP_QH_LAUNCH
    return hipGetLastError();
}

// ALGO_INDEX: the sorted index of D's band signatures from the band-major q.db_sig.T (which must hold the shape (r, nb) of D).  The
// 64-bit keys, the unsorted ranks and rocPRIM's scratch live only for the build; q.db_idx_sig / q.db_idx_rank (8 B per entry) and the
// bucket directory (one word per 2 .. 4 entries) stay.
int build_query_index(selhip_ctx* c, int nb) {
    auto& q = c->q;
    const int n_d = (int)c->n;
    const size_t total = (size_t)n_d * nb;
    DevBuf<u64> keys_in, keys_out;
    DevBuf<int> vals_in;
    DevBuf<char> tmp;
    int dir_bits = 0;                                          // 2^dir_bits buckets per band: 2 .. 4 entries each on average
    while ((4ll << dir_bits) < n_d) ++dir_bits;
    const size_t dir_words = (size_t)query_index_dir_stride(dir_bits) * nb;
    auto build = [&]() -> int {
        HIPCHK(&c->err, q.db_idx_dir.ensure(dir_words));
        HIPCHK(&c->err, q.db_idx_sig.ensure(total));
        HIPCHK(&c->err, q.db_idx_rank.ensure(total));
        HIPCHK(&c->err, keys_in.ensure(total));
        HIPCHK(&c->err, keys_out.ensure(total));
        HIPCHK(&c->err, vals_in.ensure(total));
        size_t tmp_bytes = 0;
        HIPCHK(&c->err, rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in.p, keys_out.p, vals_in.p, q.db_idx_rank.p, total, 0u, band_key_end_bit(nb), c->stream));
        HIPCHK(&c->err, tmp.ensure(tmp_bytes + 256));
        HIPCHK(&c->err, sort_band_keys(c->stream, q.db_sig.T.p, n_d, nb, keys_in.p, keys_out.p, vals_in.p, q.db_idx_rank.p, tmp.p, tmp.cap));
        hipLaunchKernelGGL(query_index_pack_kernel, dim3(grid_for((u64)total, kBlock, 8192)), dim3(kBlock), 0, c->stream,
                           keys_out.p, (long long)total, q.db_idx_sig.p);
        HIPCHK(&c->err, hipGetLastError());
        hipLaunchKernelGGL(query_index_dir_kernel, dim3(grid_for((u64)dir_words, kBlock, 8192)), dim3(kBlock), 0, c->stream,
                           q.db_idx_sig.p, n_d, nb, dir_bits, q.db_idx_dir.p);
        HIPCHK(&c->err, hipGetLastError());
        q.db_idx_dir_bits = dir_bits; q.db_idx_bands = nb;
        HIPCHK(&c->err, hipStreamSynchronize(c->stream));      // the build's own buffers go away below
        return SELHIP_OK;
    };
    const int rc = build();
    keys_in.release(); keys_out.release(); vals_in.release(); tmp.release();
    return rc;
}

// the largest query tile the stream kernel stages (qt rows of m u64 in at most 32 KiB of LDS); 0 = m too large for it
int query_stream_tile(int m) {
    const int qt = 32768 / (m * 8);
    return qt < 1 ? 0 : std::min(qt, kQStreamMaxQ);
}

// the auxiliary-HLL criterion of a query pass (kernel_query_aux.cuh), with the constants of the all-pairs pass (aux_consts).
// list == nullptr: hll_a / hll_an as the first criterion, over every query's CB window; else the hll_a stage of the two-stage
// criterion over the smh_a survivors in `list`.
hipError_t launch_query_aux(selhip_ctx* c, const selhip_int2_t* list, const u64* n_list, u64 list_cap, double tau, PassCounters* pc) {
    auto& q = c->q;
    const int n_q = (int)q.n, n_d = (int)c->n;
    const AuxConsts k = aux_consts(c->p_aux);
    const double zs = k.zs, S_sum = k.S_sum, rs = k.rs;
    const bool fma = c->fp_mode == SELHIP_FP_FMA;
    if (list) {
        const unsigned grid = grid_for(list_cap, kWave, 32768);
        with_flag(fma, [&](auto F) {
            hipLaunchKernelGGL((query_aux_list_kernel<decltype(F)::value, 1>), dim3(grid), dim3(kWave), 0, c->stream, q.d_aux_hll, c->d_aux_hll,
                               c->p_aux, n_q, list, n_list, list_cap, q.ecard.p, rs, tau, zs, S_sum, q.fin.p, (u64)q.fin.cap, &pc->n_final);
        });
        return hipGetLastError();
    }
    const int col_blocks = (n_d + kBlock - 1) / kBlock;
    const long long blocks = (long long)n_q * col_blocks;             // (bounded by the caller)
    const bool qlds = c->p_aux <= kQueryAuxLdsMaxP;
    with_flag(fma, [&](auto F) { with_flag(c->criterion == SELHIP_CRIT_HLL_AN, [&](auto AN) { with_flag(qlds, [&](auto QL) {
        hipLaunchKernelGGL((query_aux_window_kernel<decltype(F)::value, decltype(AN)::value ? 2 : 1, decltype(QL)::value>), dim3((unsigned)blocks), dim3(kBlock), 0, c->stream,
                           q.d_aux_hll, c->d_aux_hll, c->p_aux, n_q, n_d, q.lo.p, q.hi.p, col_blocks, q.ecard.p,
                           rs, tau, zs, S_sum, q.fin.p, (u64)q.fin.cap, pc);
    }); }); });
    return hipGetLastError();
}

// one query pass on the context's stream; counters land in q.h_pc (the caller waits)
// c->plan.use_index (with use_sig): ALGO_INDEX -- the probe of the sorted index in place of the signature join
int enqueue_query_pass(selhip_ctx* c, double tau) {
    auto& q = c->q;
    const int n_q = (int)q.n, n_d = (int)c->n;
    const bool smh = c->plan.smh, use_sig = c->plan.use_sig, use_index = c->plan.use_index;
    const bool none = c->criterion == SELHIP_CRIT_NONE;
    c->dominant_timer = c->timed_kernel == 1 ? T_HIST : none ? T_DENSE : !smh ? T_AUX : (use_sig ? T_JOIN : T_STAGE1);
    if (c->timing) c->timed_passes += 1;
    TimerScope total(c, T_TOTAL);
    // counter set of this pass (the other one is cleared by this pass's first kernel for the next pass)
    CounterSets::Claim pcs;
    HIPCHK(&c->err, q.pc.claim(c->stream, &pcs));       // dirty until the pass is enqueued in full
    PassCounters* const pc = pcs.cur;
    PassCounters* const pc_next = pcs.next;
    const int r = c->n_rows, nb = c->n_bands;
    const int use_cb = c->mode == SELHIP_MODE_CB_SMH ? 1 : 0;
    const unsigned win_blocks = (unsigned)((std::max(n_q, n_d) + kBlock - 1) / kBlock);
    if (use_sig) {
        // windows + the queries' band signatures in one launch
        TimerScope t(c, T_PREP);
        HIPCHK(&c->err, q.sig.ensure((size_t)n_q, (size_t)nb));
        const SigBuildShape sh = sig_build_shape(c->m, n_q, r, nb, c->sig_tile, c->sig_tile_g);
        hipLaunchKernelGGL(query_prep_sig_kernel, dim3(win_blocks + sh.blocks), dim3(kBlock), 0, c->stream, (int)win_blocks,
                           q.d_cards, n_q, c->d_cards, n_d, tau, use_cb, q.ecard.p, q.lo.p, q.hi.p, pc, pc_next,
                           q.d_aux, c->m, r, nb, pad_wave(n_q), q.sig.Q.p, q.sig.T.p, q.sig.P.p, q.sig.G.p, sh.tile_g);
        HIPCHK(&c->err, hipGetLastError());
    } else {
        TimerScope t(c, T_PREP);
        hipLaunchKernelGGL(query_windows_kernel, dim3(win_blocks), dim3(kBlock), 0, c->stream,
                           q.d_cards, n_q, c->d_cards, n_d, tau, use_cb, q.ecard.p, q.lo.p, q.hi.p, pc, pc_next);
        HIPCHK(&c->err, hipGetLastError());
    }
    {
        TimerScope t(c, T_PREP);
        // D's bit planes for stage 2a, when the all-pairs path keeps none
        if (!use_bitslices(c) && q.db_bs_gen != c->db_gen && !c->plan.emit) {
            const int rc = q.db_planes.build(&c->err, c->stream, c->d_hll, n_d);
            if (rc) return rc;
            q.db_bs_gen = c->db_gen;
        }
    }
    const BitPlanes& planes_d = use_bitslices(c) ? c->planes : q.db_planes;
    if (none) {
        if (c->dense_fused) {
            // criterion none, one launch behind the windows: records carry database ranks, nothing is left for stage 2
            {
                TimerScope t(c, T_DENSE);
                HIPCHK(&c->err, launch_dense(c->fp_mode == SELHIP_FP_FMA, c->stream, std::max(q.planes.khi, planes_d.khi),
                                             DenseSet{q.planes.bs.p, q.planes.gmax.p, q.ecard.p}, DenseSet{planes_d.bs.p, planes_d.gmax.p, q.ecard.p + n_q},
                                             n_d, q.lo.p, q.hi.p, pc, RowMap{0, n_q, n_q, 1, 0}, 0, tau, c->results.p, (u64)c->results.cap, pc, c->measure));
            }
            HIPCHK(&c->err, hipMemcpyAsync(q.h_pc, pc, sizeof(PassCounters), hipMemcpyDeviceToHost, c->stream));
            q.pc.dirty = false;
            return SELHIP_OK;
        }
        // its list route: every pair of the windows listed, then stage 2 as for every criterion
        const long long blocks = (long long)n_q * ((n_d + kEnumSpan - 1) / kEnumSpan);
        if (blocks > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
        TimerScope t(c, T_STAGE1);
        hipLaunchKernelGGL(query_enum_windows_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, n_q, q.lo.p, q.hi.p,
                           q.fin.p, (u64)q.fin.cap, &pc->n_final);
        HIPCHK(&c->err, hipGetLastError());
    } else if (!smh) {
        // hll_a / hll_an as the first criterion: straight over the windows, no signatures, no join
        if ((long long)n_q * ((n_d + kBlock - 1) / kBlock) > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
        TimerScope t(c, T_AUX);
        HIPCHK(&c->err, launch_query_aux(c, nullptr, nullptr, 0, tau, pc));
    } else if (c->plan.count) {
        // smh_c: the count kernel of the all-pairs pass over the rectangle, every query's window [lo, hi] in place of the triangle's
        TimerScope t(c, T_STAGE1);
        HIPCHK(&c->err, launch_count<true>(c, c->stream, CountSets{q.d_aux, c->d_aux, n_q, n_d, q.lo.p, q.hi.p, pc, q.ecard.p, q.ecard.p + n_q}, RowMap{0, n_q, n_q, 1, 0}, 0,
                                           q.surv.p, (u64)q.surv.cap, pc, c->plan.emit ? pc : nullptr));
        if (c->plan.emit) {
            // the count kernel wrote the records, database ranks and all: no stage 2 and no fix-up behind it
            HIPCHK(&c->err, hipMemcpyAsync(q.h_pc, pc, sizeof(PassCounters), hipMemcpyDeviceToHost, c->stream));
            q.pc.dirty = false;
            return SELHIP_OK;
        }
    } else if (use_sig) {
        const long long key = ((long long)r << 40) | ((long long)nb << 24) | ((c->db_gen & 0xFFFFF) << 1) | 1;
        if (q.db_sig_key != key) {
            // D's signatures depend on D and the band shape only: kept for the shape used last (a pass with another shape replaces them)
            TimerScope t(c, T_SIGBUILD);
            HIPCHK(&c->err, q.db_sig.ensure((size_t)n_d, (size_t)nb));
            const SigBuildShape sh = sig_build_shape(c->m, n_d, r, nb, c->sig_tile, c->sig_tile_g);
            HIPCHK(&c->err, launch_sig_kernel(c, q.db_sig, r, nb, sh, SigBuildPass{sh.blocks}));
            q.db_sig_key = key;
            q.db_sig_builds += 1;
        }
        if (use_index && q.db_idx_key != key) {
            // the index depends on D and the band shape only, like D's signatures it is sorted from: same key, same lifetime
            TimerScope t(c, T_SIGBUILD);
            q.db_idx_key = 0;
            const int rc = build_query_index(c, nb);
            if (rc) return rc;
            q.db_idx_key = key;
            q.db_idx_builds += 1;
        }
        if (use_index) {
            TimerScope t(c, T_JOIN);
            const u64 items = (u64)((n_q + kWave - 1) / kWave) * (u64)nb;          // (band, group of 64 queries), one per wave
            hipLaunchKernelGGL(query_index_probe_kernel, dim3(grid_for(items, kWavesPerBlock, 8192)), dim3(kBlock), 0, c->stream, q.sig.Q.p, q.db_sig.Q.p,
                               q.db_idx_sig.p, q.db_idx_rank.p, c->query_index_dir ? q.db_idx_dir.p : (const int*)nullptr, q.db_idx_dir_bits,
                               n_q, n_d, nb, q.lo.p, q.hi.p, q.cand.p, (u64)q.cand.cap, pc);
            HIPCHK(&c->err, hipGetLastError());
        } else {
            TimerScope t(c, T_JOIN);
            const int n_pad = pad_wave(n_d);
            const int qt = c->query_join_tile;
            const int col_blocks = (n_d + kBlock - 1) / kBlock, tiles = (n_q + qt - 1) / qt;
            const long long blocks = (long long)tiles * col_blocks;
            if (blocks > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
#define SELHIP_QJ_LAUNCH(QT) hipLaunchKernelGGL((query_sig_join_kernel<QT>), dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, q.sig.Q.p, \
                                                q.db_sig.T.p, n_q, n_d, n_pad, nb, q.lo.p, q.hi.p, col_blocks, q.cand.p, (u64)q.cand.cap, pc)
            if (qt == 16) SELHIP_QJ_LAUNCH(16);
            else          SELHIP_QJ_LAUNCH(32);
#undef SELHIP_QJ_LAUNCH
            HIPCHK(&c->err, hipGetLastError());
        }
        {
            TimerScope t(c, T_VERIFY);
            hipLaunchKernelGGL(query_verify_kernel, dim3(grid_for((u64)q.cand.cap, kBlock, 2048)), dim3(kBlock), 0, c->stream,
                               q.d_aux, c->d_aux, c->m, r, nb, n_q, q.sig.Q.p, q.db_sig.Q.p, q.cand.p, &pc->n_pre, (u64)q.cand.cap,
                               q.surv.p, (u64)q.surv.cap, pc);
            HIPCHK(&c->err, hipGetLastError());
        }
    } else {
        TimerScope t(c, T_STAGE1);
        const int qt = query_stream_tile(c->m);
        const int col_blocks = (n_d + kQStreamRows - 1) / kQStreamRows, tiles = (n_q + qt - 1) / qt;
        const long long blocks = (long long)tiles * col_blocks;
        if (blocks > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
        hipLaunchKernelGGL(query_stream_kernel, dim3((unsigned)blocks), dim3(kBlock), (size_t)qt * c->m * 8, c->stream, q.d_aux, c->d_aux, n_q, n_d,
                           c->m, r, nb, qt, q.lo.p, q.hi.p, col_blocks, q.surv.p, (u64)q.surv.cap, pc);
        HIPCHK(&c->err, hipGetLastError());
    }
    // the list stage 2 reads: the smh_a survivors, or what passed the auxiliary criterion
    const selhip_int2_t* fl = q.surv.p;
    const u64* fcnt = &pc->n_survivors;
    u64 fcap = (u64)q.surv.cap;
    if (c->criterion == SELHIP_CRIT_HLL_A_SMH_A) {
        TimerScope t(c, T_AUX);
        HIPCHK(&c->err, launch_query_aux(c, q.surv.p, &pc->n_survivors, (u64)q.surv.cap, tau, pc));
    }
    if (!survivors_final(c->criterion)) { fl = q.fin.p; fcnt = &pc->n_final; fcap = (u64)q.fin.cap; }
    // stage 2 on the combined index space: the all-pairs estimator / select kernel, unchanged
    const u64 window = (u64)q.counts.cap / 64;
    for (u64 off = 0; off < fcap; off += window) {
        {
            TimerScope t(c, T_HIST);
            HIPCHK(&c->err, launch_query_hist(c->stream, q.planes, planes_d, n_q, fl, fcnt, fcap, q.counts.p, off, window));
        }
        TimerScope t(c, T_SELECT);
        HIPCHK(&c->err, launch_select<1>(c->fp_mode == SELHIP_FP_FMA, c->stream, grid_for(std::min<u64>(window, fcap), kWave, 4096),
                                         q.counts.p, fcnt, 0, fcap, c->p, nullptr, fl, q.ecard.p, tau,
                                         c->results.p, (u64)c->results.cap, pc, nullptr, nullptr, off, window, c->measure));
    }
    hipLaunchKernelGGL(query_result_fixup_kernel, dim3(grid_for((u64)c->results.cap, kBlock, 1024)), dim3(kBlock), 0, c->stream,
                       c->results.p, &pc->n_results, (u64)c->results.cap, n_q);
    HIPCHK(&c->err, hipGetLastError());
    HIPCHK(&c->err, hipMemcpyAsync(q.h_pc, pc, sizeof(PassCounters), hipMemcpyDeviceToHost, c->stream));
    q.pc.dirty = false;
    return SELHIP_OK;
}

int ensure_query_scratch(selhip_ctx* c, size_t list_cap, size_t res_cap) {
    auto& q = c->q;
    HIPCHK(&c->err, q.lo.ensure((size_t)std::max<int64_t>(1, q.n)));
    HIPCHK(&c->err, q.hi.ensure((size_t)std::max<int64_t>(1, q.n)));
    HIPCHK(&c->err, q.ecard.ensure((size_t)std::max<int64_t>(1, q.n + c->n)));
    if (!q.pc.buf.p) { HIPCHK(&c->err, q.pc.buf.ensure(2)); q.pc.dirty = true; }
    if (!q.h_pc) HIPCHK(&c->err, hipHostMalloc((void**)&q.h_pc, sizeof(PassCounters), hipHostMallocDefault));
    size_t final_cap = list_cap;
    if (c->plan.smh) {
        HIPCHK(&c->err, q.cand.ensure(list_cap));
        HIPCHK(&c->err, q.surv.ensure(list_cap));
        final_cap = q.surv.cap;
    }
    if (!survivors_final(c->criterion)) {
        HIPCHK(&c->err, q.fin.ensure(list_cap));
        final_cap = q.fin.cap;
    }
    HIPCHK(&c->err, q.counts.ensure(std::min<size_t>(final_cap, (size_t)1 << 22) * 64));
    HIPCHK(&c->err, c->results.ensure(res_cap));
    return SELHIP_OK;
}

}  // namespace

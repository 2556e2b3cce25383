// host_pairs.hpp -- the pair-list pass of libselhip.so (selhip_ctx_run_pairs): the context's criterion over a caller's list of pairs.
// One chain on the context's stream; everything behind stage 1 (auxiliary criterion, grouping, stage 2) is the all-pairs pass's.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_pass.hpp); not a stand-alone header.
#pragma once

namespace {

// ALGO_AUTO of a list pass takes the signature route when the band shape has one and either the context already holds valid
// signatures ("sig_cache") or the list has at least n / kPairsSigShare entries.  The 2 came from bytes moved: a build reads n * 8 m
// bytes of sketches, after which an entry costs 2 * (4 n_bands + 8 n_rows) bytes; the direct route reads up to 2 * 8 m bytes per entry.
// Measured (scripts/bench_pairlist.py, profiles/pairlist_bench.json; cfg3, n = 10 000, whole pass, median of 60): direct against
// signature route 0.083 / 0.089 ms at n/8 entries, 0.091 / 0.098 at n/2, 0.160 / 0.122 at 4n -- the crossover lies near n, within
// the factor 2 of n / 2, so the constant stays.
constexpr long long kPairsSigShare = 2;

// stage-1 route of a list pass: 1 signature, 0 direct, 2 no smh_a stage ("pairs_route_used"); c->algo must already be the caller's
int pairs_route(const selhip_ctx* c, bool smh, int algo, int n_rows, int n_bands, int64_t n_pairs) {
    if (!smh) return 2;
    if (algo == SELHIP_ALGO_STREAM || !sig_supported(n_rows, n_bands)) return 0;
    if (algo == SELHIP_ALGO_SIG) return 1;
    const bool cached = c->sig_cache && c->sig_key == sig_cache_key(c, n_rows, n_bands);
    return cached || n_pairs >= c->n / kPairsSigShare ? 1 : 0;
}

hipError_t launch_pairs_filter(selhip_ctx* c, u64 off, u64 end, double tau, selhip_int2_t* out, u64 out_cap, u64* out_count, PassCounters* pc0) {
    const unsigned grid = grid_for(end - off, kPairsBlock, kPairsMaxGrid);
    if (off == 0) c->pairs_grid_used = (int)grid;                             // ("pairs_grid": of the first window)
    hipLaunchKernelGGL(pairs_filter_kernel, dim3(grid), dim3(kPairsBlock), 0, c->stream,
                       c->list_pairs, off, end, (int)c->n, c->ecard.p, tau, c->mode == SELHIP_MODE_CB_SMH ? 1 : 0, out, out_cap, out_count, pc0);
    return hipGetLastError();
}

// the whole pass (c->list_pairs / list_n, c->pairs_route_used and the run parameters are set; n > 0 and list_n > 0)
int enqueue_pairs_pass(selhip_ctx* c) {
    const int n = (int)c->n;
    const double tau = (double)c->tau_f;
    const int crit = c->criterion;
    const int use_cb = c->mode == SELHIP_MODE_CB_SMH ? 1 : 0;
    const u64 P = (u64)c->list_n;
    c->dominant_timer = c->timed_kernel == 1 ? T_HIST : T_STAGE1;
    if (c->timing) c->timed_passes += 1;
    TimerScope total(c, T_TOTAL);
    CounterSets::Claim pcs;
    HIPCHK(&c->err, c->pc.claim(c->stream, &pcs));
    c->pcb = pcs.cur;
    PassCounters* const pc0 = c->pcb;
    if (c->fail_after_flip) { c->fail_after_flip = 0; set_err(&c->err, "test hook: enqueue failed after the counter flip"); return SELHIP_E_HIP; }
    c->small_used = false;
    c->hist_image_used = 0;
    c->n_chunks_last = 1;
    // the first launch is the all-pairs pass's: truncated cards, the sortedness check, the clearing of the next pass's counters and of
    // the grouping's row counters -- over an EMPTY row range, so that no pair of the triangle is counted as evaluated
    if (c->pairs_route_used == 1) {
        HIPCHK(&c->err, launch_sig_build(c, c->n_rows, c->n_bands, tau, 0, 0, pcs.next));
    } else {
        TimerScope t(c, T_PREP);
        hipLaunchKernelGGL(cb_bounds_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream,
                           c->d_cards, n, tau, use_cb, row_map(c, 0, 0), c->ecard.p, c->hi.p, pc0,
                           grouping_on(c) && !c->plan.emit ? c->csr_cnt.p : nullptr, grouping_on(c) && !c->plan.emit ? (int)c->csr_cnt.cap : 0, 0, pcs.next,
                           c->seg_cnt.p, (int)c->seg_cnt.cap);
        HIPCHK(&c->err, hipGetLastError());
    }
    const Chain ch = chain_slices(c, 0, 1, c->stream, 0, n, pc0, false);
    const StageIO& io = ch.io;
    const selhip_int2_t* final_list = io.surv;
    const u64* final_count = &io.pc->n_survivors;
    u64 final_cap = io.cap;
    if (c->plan.smh) {
        {
            TimerScope t(c, T_STAGE1);
            const unsigned grid = grid_for(P, kPairsBlock, kPairsMaxGrid);
            c->pairs_gpw_used = 0; c->pairs_grid_used = (int)grid;            // ("pairs_gpw", "pairs_grid": the signature route's, replaced below)
            if (c->plan.count) {
                const PairsDirectShape sh = pairs_direct_shape(P);
                c->pairs_gpw_used = sh.gpw; c->pairs_grid_used = (int)sh.grid;
                c->smhc_rule_used = smhc_containment(c) ? 1 : 0;
                const PairsGammaEmit gamma_em{c->min_containment, smhc_emit(c, pc0)};
                with_flag(smhc_containment(c), [&](auto C) {
                    constexpr int RULE = decltype(C)::value ? kSmhcContainment : kSmhcFixed;
                    if (c->plan.emit)
                        hipLaunchKernelGGL((pairs_count_kernel<RULE, true>), dim3(sh.grid), dim3(kPairsBlock), 0, c->stream, c->d_aux, c->m, smhc_floor(c),
                                           c->list_pairs, P, n, c->ecard.p, tau, use_cb, sh.gpw, c->results.p, (u64)c->results.cap, &io.pc->n_survivors, pc0,
                                           gamma_em);
                    else
                        hipLaunchKernelGGL((pairs_count_kernel<RULE, false>), dim3(sh.grid), dim3(kPairsBlock), 0, c->stream, c->d_aux, c->m, c->min_matches,
                                           c->list_pairs, P, n, c->ecard.p, tau, use_cb, sh.gpw, io.surv, io.cap, &io.pc->n_survivors, pc0, c->min_containment);
                });
            } else if (c->pairs_route_used == 1)
                hipLaunchKernelGGL(pairs_verify_kernel, dim3(grid), dim3(kPairsBlock), 0, c->stream, c->d_aux, c->m, c->n_rows, c->n_bands, c->sig.Q.p,
                                   c->list_pairs, P, n, c->ecard.p, tau, use_cb, io.surv, io.cap, io.pc, pc0, c->verify_fb);
            else {
                const PairsDirectShape sh = pairs_direct_shape(P);
                c->pairs_gpw_used = sh.gpw; c->pairs_grid_used = (int)sh.grid;
                hipLaunchKernelGGL(pairs_direct_kernel<false>, dim3(sh.grid), dim3(kPairsBlock), 0, c->stream, c->d_aux, c->m, c->n_rows, c->n_bands,
                                   c->list_pairs, P, n, c->ecard.p, (const double*)nullptr, tau, use_cb, sh.gpw, io.surv, io.cap, &io.pc->n_survivors, pc0);
            }
            HIPCHK(&c->err, hipGetLastError());
        }
        if (c->plan.emit) {
            // the count kernel wrote the records: nothing is left for a stage 2
            HIPCHK(&c->err, hipMemcpyAsync(c->h_pc, c->pcb, sizeof(PassCounters) * (kMaxChunks + 1), hipMemcpyDeviceToHost, c->stream));
            c->pc.dirty = false;
            return SELHIP_OK;
        }
        if (crit == SELHIP_CRIT_HLL_A_SMH_A) {
            TimerScope t(c, T_AUX);
            HIPCHK(&c->err, launch_aux_fused<1>(c, c->stream, io.surv, &io.pc->n_survivors, io.cap, io.cap, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
            final_list = ch.fin; final_count = &io.pc->n_final; final_cap = ch.fin_cap;
        }
    } else if (crit == SELHIP_CRIT_NONE) {
        TimerScope t(c, T_STAGE1);
        HIPCHK(&c->err, launch_pairs_filter(c, 0, P, tau, io.surv, io.cap, &io.pc->n_survivors, pc0));
    } else {
        // hll_a / hll_an: the list's live entries, "enum_pairs" entries of the list at a time, each window filtered into `fin` before
        // the next overwrites it -- as the enumeration sub-passes of the all-pairs pass (a window never outgrows `cand`)
        const u64 window = std::min<u64>((u64)c->enum_pairs, (u64)c->cand.cap);
        for (u64 off = 0; off < P; off += window) {
            const u64 end = std::min(P, off + window);
            {
                TimerScope t(c, T_STAGE1);
                HIPCHK(&c->err, hipMemsetAsync(&io.pc->n_aux_in, 0, sizeof(u64), c->stream));
                HIPCHK(&c->err, launch_pairs_filter(c, off, end, tau, c->cand.p, (u64)c->cand.cap, &io.pc->n_aux_in, pc0));
            }
            TimerScope t(c, T_AUX);
            if (crit == SELHIP_CRIT_HLL_AN) HIPCHK(&c->err, launch_aux_fused<2>(c, c->stream, c->cand.p, &io.pc->n_aux_in, (u64)c->cand.cap, end - off, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
            else                            HIPCHK(&c->err, launch_aux_fused<1>(c, c->stream, c->cand.p, &io.pc->n_aux_in, (u64)c->cand.cap, end - off, tau, ch.fin, ch.fin_cap, &io.pc->n_final));
        }
        final_list = ch.fin; final_count = &io.pc->n_final; final_cap = ch.fin_cap;
    }
    const int rc = enqueue_tail(c, ch, final_list, final_count, final_cap, false, tau, pc0);
    if (rc) return rc;
    HIPCHK(&c->err, hipMemcpyAsync(c->h_pc, c->pcb, sizeof(PassCounters) * (kMaxChunks + 1), hipMemcpyDeviceToHost, c->stream));
    c->pc.dirty = false;
    return SELHIP_OK;
}

}  // namespace

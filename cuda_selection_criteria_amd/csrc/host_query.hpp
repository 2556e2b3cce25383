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
    q.own_hll.release(); q.own_aux.release(); q.own_cards.release(); q.bs.release(); q.gmax.release(); q.bs_max.release();
    q.lo.release(); q.hi.release(); q.ecard.release();
    q.sigQ.release(); q.sigT.release(); q.sigP.release(); q.sigG.release();
    q.db_sigQ.release(); q.db_sigT.release(); q.db_sigP.release(); q.db_sigG.release(); q.db_bs.release(); q.db_gmax.release();
    q.db_idx_sig.release(); q.db_idx_rank.release(); q.db_idx_dir.release();
    q.cand.release(); q.surv.release(); q.fin.release(); q.own_aux_hll.release(); q.counts.release(); q.pc.release();
    if (q.h_pc) (void)hipHostFree(q.h_pc);
    q.h_pc = nullptr;
}

// band signatures of n genomes (sig_build_kernel without its bounds blocks), into the four layouts of the builder
hipError_t launch_sig_rows(selhip_ctx* c, const u64* aux, int n, int r, int nb, uint32_t* sQ, uint32_t* sT, uint32_t* sP, uint32_t* sG) {
    if (n <= 0) return hipSuccess;
    const int n_pad = ((n + kWave - 1) / kWave) * kWave;
    const bool tile_mode = is_pow2(c->m) && is_pow2(nb) && nb <= 128 && r >= 2 && r <= 32 && c->m >= 4 && c->sig_tile;
    const long long threads = r <= kWave ? (long long)n * c->m : (long long)n * nb;
    const int tg = c->sig_tile_g;
    const unsigned blocks = tile_mode ? (unsigned)((n + tg - 1) / tg) : (unsigned)((threads + kBlock - 1) / kBlock);
    RowMap rm{0, 0, 1, 1, 0};
    hipLaunchKernelGGL(sig_build_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, aux, n, c->m, r, nb, n_pad, sQ, sT, sP, sG,
                       0, (const double*)nullptr, 0.0, 0, rm, (u64*)nullptr, (int*)nullptr, (PassCounters*)nullptr, (int*)nullptr, 0, 0,
                       (u64*)nullptr, 0, 16, (PassCounters*)nullptr, tile_mode ? tg : 0, 0);
    return hipGetLastError();
}

hipError_t ensure_sig_bufs(int n, int nb, DevBuf<uint32_t>& sQ, DevBuf<uint32_t>& sT, DevBuf<uint32_t>& sP, DevBuf<uint32_t>& sG) {
    const size_t n_pad = (((size_t)n + kWave - 1) / kWave) * kWave, half = (size_t)(nb + 1) / 2;
    hipError_t e;
    if ((e = sQ.ensure(std::max<size_t>(1, (size_t)n * nb))) != hipSuccess) return e;
    if ((e = sT.ensure(std::max<size_t>(1, n_pad * nb))) != hipSuccess) return e;
    if ((e = sP.ensure(std::max<size_t>(1, n_pad * half))) != hipSuccess) return e;
    return sG.ensure((n_pad + 2) * half);
}

hipError_t launch_query_hist(int khi, hipStream_t st, const uint32_t* bs_q, const uint8_t* gmax_q, const uint32_t* bs_d, const uint8_t* gmax_d,
                             int n_q, const selhip_int2_t* list, const u64* count, u64 cap, uint32_t* counts, u64 off, u64 window) {
    const unsigned blocks = grid_for(std::min<u64>(cap, window), kWavesPerBlock, 4096);
#define SELHIP_QH_LAUNCH(NB) hipLaunchKernelGGL((query_union_hist_kernel<NB>), dim3(blocks), dim3(kBlock), 0, st, bs_q, gmax_q, bs_d, gmax_d, n_q, \
                                                list, count, cap, counts, off, window)
    if (khi <= 16)      SELHIP_QH_LAUNCH(4);
    else if (khi <= 32) SELHIP_QH_LAUNCH(5);
    else                SELHIP_QH_LAUNCH(6);
#undef SELHIP_QH_LAUNCH
    return hipGetLastError();
}

// ALGO_INDEX: the sorted index of D's band signatures from the band-major q.db_sigT (which must hold the shape (r, nb) of D).  The
// 64-bit keys, the unsorted ranks and rocPRIM's scratch live only for the build; q.db_idx_sig / q.db_idx_rank (8 B per entry) and the
// bucket directory (one word per 2 .. 4 entries) stay.
int build_query_index(selhip_ctx* c, int nb) {
    auto& q = c->q;
    const int n_d = (int)c->n;
    const int n_pad = ((n_d + kWave - 1) / kWave) * kWave;
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
        const unsigned end_bit = 32u + (unsigned)ilog2(nb) + 1u;
        size_t tmp_bytes = 0;
        HIPCHK(&c->err, rocprim::radix_sort_pairs(nullptr, tmp_bytes, keys_in.p, keys_out.p, vals_in.p, q.db_idx_rank.p, total, 0u, end_bit, c->stream));
        HIPCHK(&c->err, tmp.ensure(tmp_bytes + 256));
        hipLaunchKernelGGL(sigkey_build_kernel, dim3((unsigned)((total + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream,
                           q.db_sigT.p, n_d, n_pad, nb, keys_in.p, vals_in.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = tmp.cap;
        HIPCHK(&c->err, rocprim::radix_sort_pairs(tmp.p, tmp_bytes, keys_in.p, keys_out.p, vals_in.p, q.db_idx_rank.p, total, 0u, end_bit, c->stream));
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

bool query_smh_stage(const selhip_ctx* c) { return c->criterion == SELHIP_CRIT_SMH_A || c->criterion == SELHIP_CRIT_HLL_A_SMH_A; }

// the auxiliary-HLL criterion of a query pass (kernel_query_aux.cuh).  zs, S and relerr_scaled come from the code launch_aux_fused
// uses, so the float / double roundings are those of the all-pairs pass.  list == nullptr: hll_a / hll_an as the first criterion,
// over every query's CB window; else the hll_a stage of the two-stage criterion over the smh_a survivors in `list`.
hipError_t launch_query_aux(selhip_ctx* c, const selhip_int2_t* list, const u64* n_list, u64 list_cap, double tau, PassCounters* pc) {
    auto& q = c->q;
    const int n_q = (int)q.n, n_d = (int)c->n;
    const float Z = 1.96f;                                   // z_score, selection.cpp:76
    const float zs_f = Z * sigma_p_of(c->p_aux);             // float * float (criteria_sketch.hpp:29,40)
    const double zs = (double)zs_f;
    const double S_sum = zs;                                 // order_n = 1 (selection.cpp:77): S = Z*sigma_p
    const double rs = relerr_scaled_for(c->p_aux);
    const bool fma = c->fp_mode == SELHIP_FP_FMA;
    if (list) {
        const unsigned grid = grid_for(list_cap, kWave, 32768);
#define SELHIP_QAL_LAUNCH(F) hipLaunchKernelGGL((query_aux_list_kernel<F, 1>), dim3(grid), dim3(kWave), 0, c->stream, q.d_aux_hll, c->d_aux_hll, \
                                                c->p_aux, n_q, list, n_list, list_cap, q.ecard.p, rs, tau, zs, S_sum, q.fin.p, (u64)q.fin.cap, &pc->n_final)
        if (fma) SELHIP_QAL_LAUNCH(true);
        else     SELHIP_QAL_LAUNCH(false);
#undef SELHIP_QAL_LAUNCH
        return hipGetLastError();
    }
    const int col_blocks = (n_d + kBlock - 1) / kBlock;
    const long long blocks = (long long)n_q * col_blocks;             // (bounded by the caller)
    const bool qlds = c->p_aux <= kQueryAuxLdsMaxP;
#define SELHIP_QAW_LAUNCH(F, CRIT, QL) hipLaunchKernelGGL((query_aux_window_kernel<F, CRIT, QL>), dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, \
                                                          q.d_aux_hll, c->d_aux_hll, c->p_aux, n_q, n_d, q.lo.p, q.hi.p, col_blocks, q.ecard.p, \
                                                          rs, tau, zs, S_sum, q.fin.p, (u64)q.fin.cap, pc)
#define SELHIP_QAW_CRIT(F, QL) do { if (c->criterion == SELHIP_CRIT_HLL_AN) SELHIP_QAW_LAUNCH(F, 2, QL); else SELHIP_QAW_LAUNCH(F, 1, QL); } while (0)
    if (fma) { if (qlds) SELHIP_QAW_CRIT(true, true);  else SELHIP_QAW_CRIT(true, false); }
    else     { if (qlds) SELHIP_QAW_CRIT(false, true); else SELHIP_QAW_CRIT(false, false); }
#undef SELHIP_QAW_CRIT
#undef SELHIP_QAW_LAUNCH
    return hipGetLastError();
}

// one query pass on the context's stream; counters land in q.h_pc (the caller waits)
// use_index (with use_sig): ALGO_INDEX -- the probe of the sorted index in place of the signature join
int enqueue_query_pass(selhip_ctx* c, bool use_sig, bool use_index, double tau) {
    auto& q = c->q;
    const int n_q = (int)q.n, n_d = (int)c->n;
    const bool smh = query_smh_stage(c);
    use_sig = use_sig && smh;
    c->dominant_timer = c->timed_kernel == 1 ? T_HIST : !smh ? T_AUX : (use_sig ? T_JOIN : T_STAGE1);
    if (c->timing) c->timed_passes += 1;
    TimerScope total(c, T_TOTAL);
    // counter set of this pass (the other one is cleared by this pass's first kernel for the next pass)
    if (q.pc_dirty) HIPCHK(&c->err, hipMemsetAsync(q.pc.p, 0, 2 * sizeof(PassCounters), c->stream));
    PassCounters* const pc = q.pc.p + q.pc_flip;
    PassCounters* const pc_next = q.pc.p + (q.pc_flip ^ 1);
    q.pc_flip ^= 1;
    q.pc_dirty = true;                                  // until the pass is enqueued in full
    const int r = c->n_rows, nb = c->n_bands;
    const int use_cb = c->mode == SELHIP_MODE_CB_SMH ? 1 : 0;
    const unsigned win_blocks = (unsigned)((std::max(n_q, n_d) + kBlock - 1) / kBlock);
    if (use_sig) {
        // windows + the queries' band signatures in one launch
        TimerScope t(c, T_PREP);
        HIPCHK(&c->err, ensure_sig_bufs(n_q, nb, q.sigQ, q.sigT, q.sigP, q.sigG));
        const bool tile_mode = is_pow2(c->m) && is_pow2(nb) && nb <= 128 && r >= 2 && r <= 32 && c->m >= 4 && c->sig_tile;
        const long long threads = r <= kWave ? (long long)n_q * c->m : (long long)n_q * nb;
        const int tg = c->sig_tile_g;
        const unsigned sig_blocks = tile_mode ? (unsigned)((n_q + tg - 1) / tg) : (unsigned)((threads + kBlock - 1) / kBlock);
        hipLaunchKernelGGL(query_prep_sig_kernel, dim3(win_blocks + sig_blocks), dim3(kBlock), 0, c->stream, (int)win_blocks,
                           q.d_cards, n_q, c->d_cards, n_d, tau, use_cb, q.ecard.p, q.lo.p, q.hi.p, pc, pc_next,
                           q.d_aux, c->m, r, nb, ((n_q + kWave - 1) / kWave) * kWave, q.sigQ.p, q.sigT.p, q.sigP.p, q.sigG.p, tile_mode ? tg : 0);
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
        if (!use_bitslices(c) && q.db_bs_gen != c->db_gen) {
            HIPCHK(&c->err, q.db_bs.ensure((size_t)n_d * kBsGenomeDwords));
            HIPCHK(&c->err, q.db_gmax.ensure((size_t)n_d));
            HIPCHK(&c->err, q.bs_max.ensure(1));
            const int rc = build_bitslices(&c->err, c->stream, c->d_hll, n_d, q.db_bs.p, q.db_gmax.p, q.bs_max.p, &q.db_khi);
            if (rc) return rc;
            q.db_bs_gen = c->db_gen;
        }
    }
    const uint32_t* const bs_d = use_bitslices(c) ? c->hll_bs.p : q.db_bs.p;
    const uint8_t* const gmax_d = use_bitslices(c) ? c->hll_gmax.p : q.db_gmax.p;
    const int khi = std::max(q.khi, use_bitslices(c) ? c->hll_khi : q.db_khi);
    if (!smh) {
        // hll_a / hll_an as the first criterion: straight over the windows, no signatures, no join
        if ((long long)n_q * ((n_d + kBlock - 1) / kBlock) > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
        TimerScope t(c, T_AUX);
        HIPCHK(&c->err, launch_query_aux(c, nullptr, nullptr, 0, tau, pc));
    } else if (use_sig) {
        const long long key = ((long long)r << 40) | ((long long)nb << 24) | ((c->db_gen & 0xFFFFF) << 1) | 1;
        if (q.db_sig_key != key) {
            // D's signatures depend on D and the band shape only: kept for the shape used last (a pass with another shape replaces them)
            TimerScope t(c, T_SIGBUILD);
            HIPCHK(&c->err, ensure_sig_bufs(n_d, nb, q.db_sigQ, q.db_sigT, q.db_sigP, q.db_sigG));
            HIPCHK(&c->err, launch_sig_rows(c, c->d_aux, n_d, r, nb, q.db_sigQ.p, q.db_sigT.p, q.db_sigP.p, q.db_sigG.p));
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
            hipLaunchKernelGGL(query_index_probe_kernel, dim3(grid_for(items, kWavesPerBlock, 8192)), dim3(kBlock), 0, c->stream, q.sigQ.p, q.db_sigQ.p,
                               q.db_idx_sig.p, q.db_idx_rank.p, c->query_index_dir ? q.db_idx_dir.p : (const int*)nullptr, q.db_idx_dir_bits,
                               n_q, n_d, nb, q.lo.p, q.hi.p, q.cand.p, (u64)q.cand.cap, pc);
            HIPCHK(&c->err, hipGetLastError());
        } else {
            TimerScope t(c, T_JOIN);
            const int n_pad = ((n_d + kWave - 1) / kWave) * kWave;
            const int qt = c->query_join_tile;
            const int col_blocks = (n_d + kBlock - 1) / kBlock, tiles = (n_q + qt - 1) / qt;
            const long long blocks = (long long)tiles * col_blocks;
            if (blocks > 0x7FFFFFFFll) { set_err(&c->err, "query pass too large for one launch"); return SELHIP_E_BADARG; }
#define SELHIP_QJ_LAUNCH(QT) hipLaunchKernelGGL((query_sig_join_kernel<QT>), dim3((unsigned)blocks), dim3(kBlock), 0, c->stream, q.sigQ.p, \
                                                q.db_sigT.p, n_q, n_d, n_pad, nb, q.lo.p, q.hi.p, col_blocks, q.cand.p, (u64)q.cand.cap, pc)
            if (qt == 16) SELHIP_QJ_LAUNCH(16);
            else          SELHIP_QJ_LAUNCH(32);
#undef SELHIP_QJ_LAUNCH
            HIPCHK(&c->err, hipGetLastError());
        }
        {
            TimerScope t(c, T_VERIFY);
            hipLaunchKernelGGL(query_verify_kernel, dim3(grid_for((u64)q.cand.cap, kBlock, 2048)), dim3(kBlock), 0, c->stream,
                               q.d_aux, c->d_aux, c->m, r, nb, n_q, q.sigQ.p, q.db_sigQ.p, q.cand.p, &pc->n_pre, (u64)q.cand.cap,
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
    if (c->criterion != SELHIP_CRIT_SMH_A) { fl = q.fin.p; fcnt = &pc->n_final; fcap = (u64)q.fin.cap; }
    // stage 2 on the combined index space: the all-pairs estimator / select kernel, unchanged
    const u64 window = (u64)q.counts.cap / 64;
    for (u64 off = 0; off < fcap; off += window) {
        {
            TimerScope t(c, T_HIST);
            HIPCHK(&c->err, launch_query_hist(khi, c->stream, q.bs.p, q.gmax.p, bs_d, gmax_d, n_q, fl, fcnt, fcap, q.counts.p, off, window));
        }
        TimerScope t(c, T_SELECT);
        HIPCHK(&c->err, launch_select<1>(c->fp_mode == SELHIP_FP_FMA, c->stream, grid_for(std::min<u64>(window, fcap), kWave, 4096),
                                         q.counts.p, fcnt, 0, fcap, c->p, nullptr, fl, q.ecard.p, tau,
                                         c->results.p, (u64)c->results.cap, pc, nullptr, nullptr, off, window));
    }
    hipLaunchKernelGGL(query_result_fixup_kernel, dim3(grid_for((u64)c->results.cap, kBlock, 1024)), dim3(kBlock), 0, c->stream,
                       c->results.p, &pc->n_results, (u64)c->results.cap, n_q);
    HIPCHK(&c->err, hipGetLastError());
    HIPCHK(&c->err, hipMemcpyAsync(q.h_pc, pc, sizeof(PassCounters), hipMemcpyDeviceToHost, c->stream));
    q.pc_dirty = false;
    return SELHIP_OK;
}

int ensure_query_scratch(selhip_ctx* c, size_t list_cap, size_t res_cap) {
    auto& q = c->q;
    HIPCHK(&c->err, q.lo.ensure((size_t)std::max<int64_t>(1, q.n)));
    HIPCHK(&c->err, q.hi.ensure((size_t)std::max<int64_t>(1, q.n)));
    HIPCHK(&c->err, q.ecard.ensure((size_t)std::max<int64_t>(1, q.n + c->n)));
    if (!q.pc.p) { HIPCHK(&c->err, q.pc.ensure(2)); q.pc_dirty = true; }
    if (!q.h_pc) HIPCHK(&c->err, hipHostMalloc((void**)&q.h_pc, sizeof(PassCounters), hipHostMallocDefault));
    size_t final_cap = list_cap;
    if (query_smh_stage(c)) {
        HIPCHK(&c->err, q.cand.ensure(list_cap));
        HIPCHK(&c->err, q.surv.ensure(list_cap));
        final_cap = q.surv.cap;
    }
    if (c->criterion != SELHIP_CRIT_SMH_A) {
        HIPCHK(&c->err, q.fin.ensure(list_cap));
        final_cap = q.fin.cap;
    }
    HIPCHK(&c->err, q.counts.ensure(std::min<size_t>(final_cap, (size_t)1 << 22) * 64));
    HIPCHK(&c->err, c->results.ensure(res_cap));
    return SELHIP_OK;
}

}  // namespace

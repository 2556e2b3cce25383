// abi_query.inc -- the C ABI of the query passes (include/selection_hip.h section 2b): upload / attach a query set and its auxiliary
// HLL sketches, run a query pass (any criterion), the top-k option of the query passes.
// Included by selection_kernels.hip.  The results go through selhip_ctx_result_count / _fetch / _stats / _last_attempts.

extern "C" {

static int after_queries(selhip_ctx* c, const double* cards_src, bool cards_on_host) {
    auto& q = c->q;
    q.planes.khi = 0;
    if (q.n == 0) { q.d_cards = nullptr; return SELHIP_OK; }
    // the registers as bit planes (stage 2a of the query pass), as for the database
    const int rc = q.planes.build(&c->err, c->stream, q.d_hll, q.n);
    if (rc) return rc;
    return load_cards(c, "query cards", q.d_hll, q.n, cards_src, cards_on_host, q.own_cards, &q.d_cards);
}

static int check_query_shape(selhip_ctx* c, int64_t n_q) {
    if (!c->d_aux && c->n) { set_err(&c->err, "upload or attach the database before the queries"); return SELHIP_E_STATE; }
    if (c->m <= 0) { set_err(&c->err, "upload or attach the database before the queries"); return SELHIP_E_STATE; }
    if (c->p != 14) { set_err(&c->err, "query passes need p = 14 sketches (the database has p = %d)", c->p); return SELHIP_E_BADARG; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    if (n_q < 0 || n_q > 0x7FFFFFF0ll) { set_err(&c->err, "n_q %lld out of range", (long long)n_q); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

int selhip_ctx_upload_queries(selhip_ctx* c, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards, int64_t n_q) {
    if (!c) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = check_query_shape(c, n_q);
    if (rc) return rc;
    if (n_q > 0 && (!h_hll || !h_aux)) { set_err(&c->err, "null query sketch pointer"); return SELHIP_E_BADARG; }
    auto& q = c->q;
    q.n = -1;
    q.d_aux_hll = nullptr; q.p_aux = 0;                 // a new query set never meets the previous one's auxiliary sketches
    if (n_q > 0) {
        HIPCHK(&c->err, q.own_hll.ensure((size_t)n_q << 14));
        HIPCHK(&c->err, q.own_aux.ensure((size_t)n_q * c->m));
        HIPCHK(&c->err, hipMemcpyAsync(q.own_hll.p, h_hll, (size_t)n_q << 14, hipMemcpyHostToDevice, c->stream));
        HIPCHK(&c->err, hipMemcpyAsync(q.own_aux.p, h_aux, (size_t)n_q * c->m * 8, hipMemcpyHostToDevice, c->stream));
    }
    q.d_hll = q.own_hll.p; q.d_aux = q.own_aux.p;
    q.n = n_q;
    rc = after_queries(c, h_cards, true);
    if (rc) q.n = -1;
    return rc;
}

int selhip_ctx_attach_queries(selhip_ctx* c, const uint8_t* d_hll, const uint64_t* d_aux, const double* d_cards, int64_t n_q) {
    if (!c) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = check_query_shape(c, n_q);
    if (rc) return rc;
    if (n_q > 0 && (!d_hll || !d_aux)) { set_err(&c->err, "null query sketch pointer"); return SELHIP_E_BADARG; }
    if (((uintptr_t)d_hll & 15) || ((uintptr_t)d_aux & 15)) { set_err(&c->err, "query sketch pointers must be 16-byte aligned"); return SELHIP_E_BADARG; }
    auto& q = c->q;
    q.d_aux_hll = nullptr; q.p_aux = 0;
    q.d_hll = d_hll; q.d_aux = (const u64*)d_aux;
    q.n = n_q;
    rc = after_queries(c, d_cards, false);
    if (rc) q.n = -1;
    return rc;
}

static int check_query_aux(selhip_ctx* c, const void* p, int p_aux) {
    if (c->q.n < 0) { set_err(&c->err, "upload or attach the queries before their auxiliary HLL sketches"); return SELHIP_E_STATE; }
    if (p_aux < 4 || p_aux > kMaxAuxP) { set_err(&c->err, "p_aux %d out of range [4,%d]", p_aux, kMaxAuxP); return SELHIP_E_BADARG; }
    if (!p && c->q.n > 0) { set_err(&c->err, "null query auxiliary HLL pointer"); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

int selhip_ctx_upload_queries_aux_hll(selhip_ctx* c, const uint8_t* h_aux_hll, int p_aux) {
    if (!c) return SELHIP_E_BADARG;
    int rc = check_query_aux(c, h_aux_hll, p_aux);
    if (rc) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    auto& q = c->q;
    q.d_aux_hll = nullptr; q.p_aux = 0;
    return upload_aux_hll_rows(c, h_aux_hll, q.n, p_aux, q.own_aux_hll, &q.d_aux_hll, &q.p_aux);
}

int selhip_ctx_attach_queries_aux_hll(selhip_ctx* c, const uint8_t* d_aux_hll, int p_aux) {
    if (!c) return SELHIP_E_BADARG;
    int rc = check_query_aux(c, d_aux_hll, p_aux);
    if (rc) return rc;
    if ((uintptr_t)d_aux_hll & 15) { set_err(&c->err, "query auxiliary HLL pointer must be 16-byte aligned"); return SELHIP_E_BADARG; }
    auto& q = c->q;
    if (!d_aux_hll) {                                   // (n_q == 0: nothing to point at)
        HIPCHK(&c->err, q.own_aux_hll.ensure(1));
        d_aux_hll = q.own_aux_hll.p;
    }
    q.d_aux_hll = d_aux_hll; q.p_aux = p_aux;
    return SELHIP_OK;
}

int selhip_ctx_fold_queries_aux_hll(selhip_ctx* c, int p_aux) {
    if (!c) return SELHIP_E_BADARG;
    auto& q = c->q;
    int rc = check_query_aux(c, q.d_hll, p_aux);           // (the main rows stand in for the pointer: null only for an empty set)
    if (rc) return rc;
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    rc = check_fold_p(c, p_aux);
    if (rc) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    q.d_aux_hll = nullptr; q.p_aux = 0;
    return fold_aux_hll_rows(c, q.d_hll, q.n, p_aux, q.own_aux_hll, &q.d_aux_hll, &q.p_aux);
}

int selhip_ctx_run_queries(selhip_ctx* c, int mode, int algo, float tau_f, int n_rows, int n_bands) {
    if (!c) return SELHIP_E_BADARG;
    auto& q = c->q;
    if (q.n < 0) { set_err(&c->err, "run_queries before upload / attach of the queries"); return SELHIP_E_STATE; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    if (mode != SELHIP_MODE_SMH && mode != SELHIP_MODE_CB_SMH) { set_err(&c->err, "bad mode %d", mode); return SELHIP_E_BADARG; }
    { const int rc = accept_measure(c, mode); if (rc) return rc; }
    { const int rc = accept_estimator(c); if (rc) return rc; }
    if (c->criterion == SELHIP_CRIT_NONE) { const int rc = accept_dense(c); if (rc) return rc; }
    if (c->criterion == SELHIP_CRIT_SMH_C) { const int rc = accept_count(c); if (rc) return rc; }
    if (aux_criterion(c->criterion)) {
        // the auxiliary HLL sketches of both sets, with one precision
        if ((c->n && !c->d_aux_hll) || (q.n && !q.d_aux_hll)) {
            set_err(&c->err, "criterion %d needs the auxiliary HLL sketches of the database (selhip_ctx_upload_aux_hll) and of the queries "
                             "(selhip_ctx_upload_queries_aux_hll)", c->criterion);
            return SELHIP_E_STATE;
        }
        if (c->d_aux_hll && q.d_aux_hll && c->p_aux != q.p_aux) {
            set_err(&c->err, "auxiliary HLL precision of the queries (%d) != that of the database (%d)", q.p_aux, c->p_aux);
            return SELHIP_E_BADARG;
        }
    }
    const PassPlan plan = pass_plan(c->criterion, algo, c->m, n_rows, n_bands, c->estimator);
    const bool smh = plan.smh;
    if (algo != SELHIP_ALGO_AUTO && algo != SELHIP_ALGO_STREAM && algo != SELHIP_ALGO_SIG && algo != SELHIP_ALGO_HASHJOIN && algo != SELHIP_ALGO_INDEX) { set_err(&c->err, "bad algo %d", algo); return SELHIP_E_BADARG; }
    if (smh && !plan.count) {
        // (hll_a / hll_an alone and smh_c read neither n_rows / n_bands nor algo, as in selhip_ctx_run_async)
        if (algo == SELHIP_ALGO_HASHJOIN) { set_err(&c->err, "query passes have no ALGO_HASHJOIN; use AUTO, SIG, STREAM or INDEX"); return SELHIP_E_BADARG; }
        if (n_rows <= 0 || n_bands <= 0 || (long long)n_rows * n_bands != c->m) {
            set_err(&c->err, "n_rows*n_bands (%d*%d) != m (%d)", n_rows, n_bands, c->m);
            return SELHIP_E_BADARG;
        }
        if (plan.bad) { set_err(&c->err, plan.bad, n_rows, n_bands); return SELHIP_E_BADARG; }
        if (!plan.use_sig && query_stream_tile(c->m) == 0) { set_err(&c->err, "ALGO_STREAM of a query pass holds m <= 4096 buckets (m = %d)", c->m); return SELHIP_E_BADARG; }
    }
    HIPCHK(&c->err, hipSetDevice(c->device));
    c->mode = mode; c->algo = algo; c->tau_f = tau_f; c->n_rows = n_rows; c->n_bands = n_bands; c->plan = plan;
    c->have_run = false;
    std::memset(&c->last, 0, sizeof c->last);
    c->last_was_query = true;
    c->topk_applied = false; c->topk_n = 0;
    if (q.n == 0 || c->n == 0) { c->have_run = true; c->last_attempts = 1; c->topk_applied = c->query_topk > 0; return SELHIP_OK; }
    const size_t have = smh ? q.surv.cap : q.fin.cap;
    size_t cap = std::max<size_t>(have, std::max<size_t>((size_t)1 << 16, (size_t)q.n * 16));
    if (c->init_cap > 0) cap = std::max<size_t>(have, (size_t)c->init_cap);             // test hook: start small, grow on overflow
    size_t res_cap = std::max<size_t>(c->results.cap, cap);
    const double tau = (double)tau_f;                 // float threshold widened, selection.cpp:81,164
    for (int attempt = 0; attempt < kMaxAttempts; ++attempt) {
        int rc = ensure_query_scratch(c, cap, res_cap);
        if (!rc) rc = enqueue_query_pass(c, tau);
        if (rc) return rc;
        HIPCHK(&c->err, wait_stream(c->stream));
        const PassCounters pc = *q.h_pc;
        if (pc.unsorted) { set_err(&c->err, "database or query cards are not in ascending order"); return SELHIP_E_BADARG; }
        bool grow = false;
        // (n_pre: the join's list; n_survivors: the survivor list; n_final: what passed the auxiliary criterion)
        const u64 worst = std::max(std::max(pc.n_pre, pc.n_survivors), !survivors_final(c->criterion) ? pc.n_final : 0);
        if (plan.emit) {
            // (stage 1 stored nothing but records: n_survivors is a tally)
        } else if ((smh && (worst > q.surv.cap || worst > q.cand.cap)) || (!survivors_final(c->criterion) && worst > q.fin.cap)) {
            cap = std::max(cap, grown(worst));
            grow = true;
        }
        if (results_overflowed(pc.n_results, c->results.cap, &res_cap)) grow = true;
        if (!grow) {
            c->last = pc; c->have_run = true; c->last_attempts = attempt + 1; c->last_was_query = true;
            if (c->criterion == SELHIP_CRIT_NONE) dense_stats(&c->last);
            if (c->query_topk > 0) {
                // the pass is accepted and n_results known: every query keeps its K best, on the same stream
                rc = reduce_topk(c, {c->query_topk, c->q.n, false, "query", "queries"});
                if (rc) { c->have_run = false; return rc; }
                c->topk_applied = true;
            }
            return SELHIP_OK;
        }
        res_cap = std::max(res_cap, cap);               // an internal list was too small: counts are exact, grow once and repeat
    }
    set_err(&c->err, "output buffers kept overflowing");
    return SELHIP_E_OVERFLOW;
}

int selhip_ctx_set_query_topk(selhip_ctx* c, int k) {
    if (!c) return SELHIP_E_BADARG;
    if (k < 0 || k > SELHIP_TOPK_MAX) { set_err(&c->err, "query top-k must be 0 (off) or in [1, %d] (got %d)", SELHIP_TOPK_MAX, k); return SELHIP_E_BADARG; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->query_topk = k;
    return SELHIP_OK;
}

int selhip_ctx_fetch_ranked(selhip_ctx* c, selhip_pair_t* h_out, int64_t cap) {
    if (!c || (cap > 0 && !h_out) || cap < 0) return SELHIP_E_BADARG;
    if (!c->have_run || !c->topk_applied) {
        set_err(&c->err, "fetch_ranked needs a finished query pass with top-k on (selhip_ctx_set_query_topk) or a finished all-pairs pass "
                         "with top-k on (selhip_ctx_set_allpairs_topk)");
        return SELHIP_E_STATE;
    }
    const int64_t cnt = c->topk_n;
    if (cnt == 0) return SELHIP_OK;
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, hipMemcpyAsync(h_out, c->results.p, (size_t)std::min(cnt, cap) * sizeof(selhip_pair_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return cnt > cap ? SELHIP_E_OVERFLOW : SELHIP_OK;
}

}  // extern "C"

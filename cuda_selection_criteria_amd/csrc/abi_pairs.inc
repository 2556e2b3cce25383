// abi_pairs.inc -- the C ABI of the pair-list passes (include/selection_hip.h section 2e): selhip_ctx_run_pairs / _run_pairs_async.
// selhip_ctx_finish (abi_context.inc) waits for the pass, reports invalid entries and repeats it when a list was too small.
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_run_pairs_async(selhip_ctx* c, const selhip_int2_t* d_pairs, int64_t n_pairs,
                               int mode, int algo, float tau_f, int n_rows, int n_bands) {
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    if (n_pairs < 0 || n_pairs > 0x7FFFFFFFll) { set_err(&c->err, "n_pairs %lld outside [0, 2^31 - 1]", (long long)n_pairs); return SELHIP_E_BADARG; }
    if (n_pairs > 0 && !d_pairs) { set_err(&c->err, "null pair list"); return SELHIP_E_BADARG; }
    if ((uintptr_t)d_pairs & 7) { set_err(&c->err, "the pair list must be 8-byte aligned"); return SELHIP_E_BADARG; }
    if (!c->d_aux && (c->n || n_pairs)) { set_err(&c->err, "run before upload/attach"); return SELHIP_E_STATE; }
    if (mode != SELHIP_MODE_SMH && mode != SELHIP_MODE_CB_SMH) { set_err(&c->err, "bad mode %d", mode); return SELHIP_E_BADARG; }
    { const int rc = accept_measure(c, mode); if (rc) return rc; }
    { const int rc = accept_estimator(c); if (rc) return rc; }
    if (algo == SELHIP_ALGO_HASHJOIN || algo == SELHIP_ALGO_INDEX) {
        set_err(&c->err, "a pair-list pass takes SELHIP_ALGO_AUTO, _SIG or _STREAM: algo %d is a join, not a check of a given pair", algo);
        return SELHIP_E_BADARG;
    }
    if (algo != SELHIP_ALGO_AUTO && algo != SELHIP_ALGO_STREAM && algo != SELHIP_ALGO_SIG) { set_err(&c->err, "bad algo %d", algo); return SELHIP_E_BADARG; }
    if (c->allpairs_topk > 0) {
        set_err(&c->err, "a pair-list pass has no all-pairs top-k (an entry may be listed twice, so partners are not unique per owner): selhip_ctx_set_allpairs_topk(ctx, 0) first");
        return SELHIP_E_STATE;
    }
    if (c->il_parts > 1) { set_err(&c->err, "a pair-list pass takes no row interleave (it describes a triangle): shard the list itself"); return SELHIP_E_STATE; }
    if (c->cand_begin > 0) { set_err(&c->err, "a pair-list pass takes no candidate begin (it describes a triangle): shard the list itself"); return SELHIP_E_STATE; }
    if (aux_criterion(c->criterion) && !c->d_aux_hll && c->n) {
        set_err(&c->err, "criterion %d needs auxiliary HLL sketches (selhip_ctx_upload_aux_hll)", c->criterion);
        return SELHIP_E_STATE;
    }
    if (c->criterion == SELHIP_CRIT_NONE) {
        const int route = c->dense_route_used;                   // (a list pass runs neither route of the all-pairs pass)
        const int rc = accept_dense(c);
        c->dense_route_used = route;
        if (rc) return rc;
    }
    if (c->criterion == SELHIP_CRIT_SMH_C) { const int rc = accept_count(c); if (rc) return rc; }
    // (which stage 1 the criterion has: pass_plan's answer; the route below replaces its choice among the smh_a algorithms)
    PassPlan plan;
    { const PassPlan pp = pass_plan(c->criterion, SELHIP_ALGO_STREAM, c->m, n_rows, n_bands); plan.smh = pp.smh; plan.count = pp.count; plan.emit = pp.count && c->estimator == SELHIP_ESTIMATOR_SMH; }
    if (plan.smh && !plan.count && (n_rows <= 0 || n_bands <= 0 || (long long)n_rows * n_bands != c->m)) {
        set_err(&c->err, "n_rows*n_bands (%d*%d) != m (%d)", n_rows, n_bands, c->m);
        return SELHIP_E_BADARG;
    }
    if (plan.smh && !plan.count && algo == SELHIP_ALGO_SIG && !sig_supported(n_rows, n_bands)) {
        set_err(&c->err, "ALGO_SIG needs power-of-two rows and 8..128 bands (got %d x %d)", n_rows, n_bands);
        return SELHIP_E_BADARG;
    }
    HIPCHK(&c->err, hipSetDevice(c->device));
    // (the route first: the cache key asks join_sliced, which reads the algorithm of the pass -- SIG and STREAM are alike to it)
    c->algo = SELHIP_ALGO_SIG;
    const int route = plan.count ? 0 : pairs_route(c, plan.smh, algo, n_rows, n_bands, n_pairs);      // (the count has the direct route only)
    plan.use_sig = route == 1;
    c->mode = mode; c->algo = route == 1 ? SELHIP_ALGO_SIG : SELHIP_ALGO_STREAM; c->tau_f = tau_f; c->n_rows = n_rows; c->n_bands = n_bands; c->plan = plan;
    c->row_begin = 0; c->row_end = c->n;
    c->have_run = false; c->last_was_query = false; c->topk_applied = false; c->topk_n = 0;
    c->rd.on = false;                                              // (a pair-list pass does not read selhip_ctx_set_topk_rounds)
    c->list_pass = true; c->list_pairs = d_pairs; c->list_n = n_pairs; c->pairs_route_used = route;
    c->pairs_gpw_used = 0; c->pairs_grid_used = 0;                 // (enqueue_pairs_pass sets both; an empty list launches nothing)
    c->small_used = false; c->n_chunks_last = 1;
    std::memset(&c->last, 0, sizeof c->last);
    if (n_pairs == 0) { c->pending = false; c->have_run = true; c->last_attempts = 1; return SELHIP_OK; }
    if (c->n == 0) {
        set_err(&c->err, "the pair list holds %lld invalid entries (x == y, or a rank outside [0, 0)); entry 0 is one", (long long)n_pairs);
        return SELHIP_E_BADARG;
    }
    size_t surv_cap = std::max<size_t>(c->surv.cap, std::max<size_t>((size_t)1 << 20, (size_t)c->n * 16));
    if (c->init_cap > 0) surv_cap = std::max<size_t>(c->surv.cap, (size_t)c->init_cap);       // test hook: start small, grow on overflow
    const size_t res_cap = std::max<size_t>(c->results.cap, surv_cap);
    int rc = ensure_scratch(c, surv_cap, res_cap);
    if (rc) return rc;
    rc = enqueue_pairs_pass(c);
    if (rc) return rc;
    c->pending = true;
    return SELHIP_OK;
}

int selhip_ctx_run_pairs(selhip_ctx* c, const selhip_int2_t* d_pairs, int64_t n_pairs,
                         int mode, int algo, float tau_f, int n_rows, int n_bands) {
    const int rc = selhip_ctx_run_pairs_async(c, d_pairs, n_pairs, mode, algo, tau_f, n_rows, n_bands);
    if (rc) return rc;
    return selhip_ctx_finish(c);
}

}  // extern "C"

// abi_context.inc -- the C ABI of the context (include/selection_hip.h sections 1-2): create / destroy, parameters, upload / attach,
// run / finish, results, timing.  Included by selection_kernels.hip.

// =============================================================================================
// C ABI
// =============================================================================================
extern "C" {

const char* selhip_version(void) { return "selhip 0.1 (gfx950)"; }

int selhip_device_count(void) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess) return 0;
    return cnt;
}

const char* selhip_last_error(const selhip_ctx* ctx) {
    if (ctx) return ctx->err.c_str();
    return g_last_error.c_str();
}

int selhip_ctx_create(selhip_ctx** out, int device) {
    if (!out) return SELHIP_E_BADARG;
    *out = nullptr;
    int rc = check_device(nullptr);
    if (rc) return rc;
    int cnt = 0;
    (void)hipGetDeviceCount(&cnt);
    if (device < 0 || device >= cnt) { set_err(nullptr, "device %d out of range (0..%d)", device, cnt - 1); return SELHIP_E_BADARG; }
    HIPCHK(nullptr, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(nullptr, hipGetDeviceProperties(&prop, device));
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_err(nullptr, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
        return SELHIP_E_NODEVICE;
    }
    selhip_ctx* c = new selhip_ctx();
    c->device = device;
    c->dev_cus = prop.multiProcessorCount;
    *out = c;
    return SELHIP_OK;
}

void selhip_ctx_destroy(selhip_ctx* c) {
    if (!c) return;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    drain_timers(c);
    c->own_hll.release(); c->own_aux.release(); c->own_cards.release();
    c->ecard.release(); c->hi.release(); c->pc.buf.release(); c->seg_cnt.release(); c->surv.release();
    c->counts.release(); c->results.release(); c->self_pairs.release();
    c->aux_il.release(); c->cand.release(); c->sig.release(); c->fin.release(); c->own_aux_hll.release();
    c->hj_keys_in.release(); c->hj_keys_out.release(); c->hj_vals_in.release(); c->hj_vals_out.release(); c->hj_tmp.release();
    c->csr_cnt.release(); c->csr_start.release(); c->grouped.release(); c->scan_tmp.release();
    c->planes.release(); c->small_bar.release(); c->mat_row_pos.release(); c->mat_col_pos.release();
    c->hll_sparse.release(); c->hll_sparse_dev_t.release(); c->hll_image.release();
    release_queries(c);
    release_topk(c);
    c->gs.release();
    release_merge(c);
    if (c->h_pc) (void)hipHostFree(c->h_pc);
    if (c->st_stage1) {
        (void)hipStreamDestroy(c->st_stage1);
        (void)hipEventDestroy(c->ev_start); (void)hipEventDestroy(c->ev_end);
    }
    delete c;
}

int selhip_ctx_set_stream(selhip_ctx* c, void* hip_stream) {
    if (!c) return SELHIP_E_BADARG;
    if (c->stream != (hipStream_t)hip_stream && c->pc.buf.p) {
        // the counter sets were cleared by work on the old stream, which the new one is not ordered behind
        (void)hipStreamSynchronize(c->stream);
        c->pc.dirty = true;
    }
    c->stream = (hipStream_t)hip_stream;
    return SELHIP_OK;
}

int selhip_ctx_set_fp_mode(selhip_ctx* c, int fp_mode) {
    if (!c || (fp_mode != SELHIP_FP_FMA && fp_mode != SELHIP_FP_STRICT)) return SELHIP_E_BADARG;
    c->fp_mode = fp_mode;
    return SELHIP_OK;
}

int selhip_ctx_set_row_interleave(selhip_ctx* c, int block_rows, int n_parts, int part) {
    if (!c) return SELHIP_E_BADARG;
    if (n_parts <= 1) { c->il_parts = 1; c->il_part = 0; return SELHIP_OK; }
    if (block_rows < 32 || block_rows % 32 || part < 0 || part >= n_parts) {
        set_err(&c->err, "row interleave: block_rows must be a multiple of 32 (>= 32) and 0 <= part < n_parts");
        return SELHIP_E_BADARG;
    }
    c->il_block = block_rows; c->il_parts = n_parts; c->il_part = part;     // (the join's tile height is fitted to the block in join_tile_rows)
    return SELHIP_OK;
}

// Names beyond the documented ones (include/selection_hip.h) -- hooks of the test-suite and measurement knobs, not interface:
//   "verify_fb"        1 sends every candidate through the hash-collision fallback of the verification
//   "init_cap"         initial capacity of the candidate / survivor / result lists (they grow and the pass repeats)
//   "enum_pairs"       pairs listed per sub-pass when hll_a / hll_an is the first criterion (default 2^26)
//   "fail_after_flip"  the next enqueue fails right after claiming its counter set (recovery of the double-buffered counters)
//   "small_pass" = 3   the one-launch pass with NO patience at its grid barrier (the bounded wait running out -> regular path)
//   "sig_tile_g"       genomes per tile of the tiled signature build (8 / 16 / 32; 16 is the measured optimum)
//   "hist_pad"         extra LDS bytes per block of the byte-row stage-2a kernel (lowers the resident waves per CU)
//   "query_join_tile"  queries per block of the query passes' signature join (16, the default, or 32)
//   "query_index_dir"  ALGO_INDEX: 1 (default) the probe starts from the index's bucket directory, 0 it searches the whole band segment
int selhip_ctx_set_param(selhip_ctx* c, const char* name, int value) {
    if (!c || !name) return SELHIP_E_BADARG;
    if (!std::strcmp(name, "query_index_dir")) { c->query_index_dir = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "join_qt")) {
        if (value != 0 && (value < 16 || value > 4096 || value % 16)) { set_err(&c->err, "join_qt must be 0 (automatic) or a multiple of 16 in [16, 4096]"); return SELHIP_E_BADARG; }
        c->join_qt = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "verify_fb")) { c->verify_fb = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "fail_after_flip")) { c->fail_after_flip = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "join_wpb")) {
        if (value != 1 && value != 4 && value != 8) { set_err(&c->err, "join_wpb must be 1, 4 or 8"); return SELHIP_E_BADARG; }
        c->join_wpb = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "join_form")) {
        if (value < 0 || value > 2) { set_err(&c->err, "join_form must be 0 (packed minimum), 1 (zero-half) or 2 (bit-sliced)"); return SELHIP_E_BADARG; }
        c->join_form = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "join_t")) {
        if (value < 0 || value > 2) { set_err(&c->err, "join_t must be 0 (automatic), 1 or 2"); return SELHIP_E_BADARG; }
        c->join_t = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "join_tri")) { c->join_tri = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "join_db")) { c->join_db = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "join_q")) { c->join_q = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "sig_tile")) { c->sig_tile = value != 0; c->sig_key = 0; return SELHIP_OK; }
    if (!std::strcmp(name, "sig_tile_g")) {
        if (value != 8 && value != 16 && value != 32) { set_err(&c->err, "sig_tile_g must be 8, 16 or 32"); return SELHIP_E_BADARG; }
        c->sig_tile_g = value; c->sig_key = 0;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "sig_cache")) { c->sig_cache = value != 0; c->sig_key = 0; return SELHIP_OK; }
    if (!std::strcmp(name, "enum_pairs")) {
        if (value < 1) { set_err(&c->err, "enum_pairs must be >= 1"); return SELHIP_E_BADARG; }
        c->enum_pairs = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "init_cap")) {
        if (value < 0) { set_err(&c->err, "init_cap must be >= 0"); return SELHIP_E_BADARG; }
        c->init_cap = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "join_bits")) {
        if (value != 15 && value != 16 && value != 32) { set_err(&c->err, "join_bits must be 15, 16 or 32"); return SELHIP_E_BADARG; }
        c->join_bits = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "small_pass")) {
        if (value < -1 || value > 3) { set_err(&c->err, "small_pass must be -1 (automatic), 0 (off), 1 or 2 (1 through hipLaunchCooperativeKernel)"); return SELHIP_E_BADARG; }
        c->small_pass = value; c->small_pass_failed = false;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "group_min_n")) {
        if (value < 0) { set_err(&c->err, "group_min_n must be >= 0"); return SELHIP_E_BADARG; }
        c->group_min_n = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "group_label")) {
        if (value < -1 || value > 1) { set_err(&c->err, "group_label must be -1 (automatic), 0 or 1"); return SELHIP_E_BADARG; }
        c->group_label = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_run")) {
        if (value < 0 || value > 1024) { set_err(&c->err, "hist_run must be in [0, 1024] (0 = automatic)"); return SELHIP_E_BADARG; }
        c->hist_run = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_pad")) {
        if (value < 0 || value > 48 * 1024) { set_err(&c->err, "hist_pad must be in [0, 49152]"); return SELHIP_E_BADARG; }
        c->hist_pad = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "query_join_tile")) {
        if (value != 16 && value != 32) { set_err(&c->err, "query_join_tile must be 16 or 32"); return SELHIP_E_BADARG; }
        c->query_join_tile = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "timed_kernel")) {
        if (value < 0 || value > 1) { set_err(&c->err, "timed_kernel must be 0 (stage-1 kernel) or 1 (stage 2a)"); return SELHIP_E_BADARG; }
        c->timed_kernel = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_algo")) {
        // takes effect at the next selhip_ctx_upload / _attach (the bit planes are written there)
        if (value < -1 || value > 1) { set_err(&c->err, "hist_algo must be -1 (automatic), 0 (byte rows, LDS histogram) or 1 (bit planes)"); return SELHIP_E_BADARG; }
        c->hist_algo = value;
        if (value == 0) c->planes.khi = 0;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_sparse")) {
        if (value < -1 || value > 1) { set_err(&c->err, "hist_sparse must be -1 (automatic), 0 (every value from the bit planes) or 1 (values >= the set's threshold from its sparse lists)"); return SELHIP_E_BADARG; }
        c->hist_sparse = value;
        return SELHIP_OK;
    }
    // (not part of the documented interface: 0 = stage 2a reads the six-plane rows even where the set holds a clamped image; -1 and 1 read
    //  the image wherever it is exact -- with the lists in use at a threshold of 4, 8 or 12; the same counts either way)
    if (!std::strcmp(name, "hist_image")) {
        if (value < -1 || value > 1) { set_err(&c->err, "hist_image must be -1 (automatic), 0 (the six-plane rows) or 1 (the clamped image where the set holds one)"); return SELHIP_E_BADARG; }
        c->hist_image = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "dense_fused")) { c->dense_fused = value != 0; return SELHIP_OK; }
    if (!std::strcmp(name, "matrix_mirror")) { c->matrix_mirror = value != 0; return SELHIP_OK; }   // measurement switch: 0 = no mirrored stores
    // (not part of the documented interface: the measurement switch of scripts/bench_matrix_smh.py -- 1 = a self matrix of the SuperMinHash
    //  measures computes every pair once and mirrors it, 3 = it computes the whole square; the same matrix either way)
    if (!std::strcmp(name, "matrix_smh_form")) {
        if (value != 1 && value != 3) { set_err(&c->err, "matrix_smh_form: 1 (every pair once, mirrored) or 3 (the whole square)"); return SELHIP_E_BADARG; }
        c->matrix_smh_form = (int)value; return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_dense_degree")) {
        if (value < -1 || value > (1 << 20)) { set_err(&c->err, "hist_dense_degree must be in [-1, 2^20] (-1 = never)"); return SELHIP_E_BADARG; }
        c->hist_dense_degree = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_bs_blocks")) {
        if (value < 8 || value > 65536 || value % 8) { set_err(&c->err, "hist_bs_blocks must be a multiple of 8 in [8, 65536]"); return SELHIP_E_BADARG; }
        c->hist_bs_blocks = value;
        return SELHIP_OK;
    }
    if (!std::strcmp(name, "hist_blocks")) {
        if (value < 8 || value > 65536 || value % 8) { set_err(&c->err, "hist_blocks must be a multiple of 8 in [8, 65536]"); return SELHIP_E_BADARG; }
        c->hist_blocks = value;
        return SELHIP_OK;
    }
    // (a test hook, not part of the documented interface, and PROCESS-wide -- selhip_components has no context: > 0 fixes the grid of
    //  cluster_edges_kernel for every cluster / components call that follows, 0 = sized from the list; the same clusters either way.
    //  The record kernels of the greedy clusters, kernel_greedy.cuh, take their grid from the same function and so from this hook)
    if (!std::strcmp(name, "cluster_blocks")) {
        if (value < 0 || value > 65536) { set_err(&c->err, "cluster_blocks must be in [0, 65536] (0 = automatic)"); return SELHIP_E_BADARG; }
        g_cluster_blocks.store(value, std::memory_order_relaxed);
        return SELHIP_OK;
    }
    // (its sibling, as process-wide and as little part of the documented interface: > 0 fixes the grid of every kernel that takes a lane
    //  per vertex, row or slot -- whatever cluster_vertex_grid sizes: clusters, greedy, forest, linkage, the merge's row kernels -- so that
    //  a small n walks their grid-stride loops many times; 0 = sized from n; the same answers either way)
    if (!std::strcmp(name, "vertex_blocks")) {
        if (value < 0 || value > 65536) { set_err(&c->err, "vertex_blocks must be in [0, 65536] (0 = automatic)"); return SELHIP_E_BADARG; }
        g_vertex_blocks.store(value, std::memory_order_relaxed);
        return SELHIP_OK;
    }
    set_err(&c->err, "unknown parameter '%s'", name);
    return SELHIP_E_BADARG;
}

int selhip_ctx_get_param(const selhip_ctx* c, const char* name, int* value) {
    if (!c || !name || !value) return SELHIP_E_BADARG;
    if (!std::strcmp(name, "hll_khi"))          { *value = c->planes.khi; return SELHIP_OK; }             // largest p = 14 register value + 1 (0: no bit planes)
    if (!std::strcmp(name, "hist_bitplanes"))   { *value = use_bitslices(c) ? 1 : 0; return SELHIP_OK; }
    if (!std::strcmp(name, "hist_sparse_t"))    { *value = sparse_t_used(c); return SELHIP_OK; }      // threshold of the all-pairs stage 2a's sparse lists, 0 = off
    if (!std::strcmp(name, "hist_image"))       { *value = c->hist_image_used; return SELHIP_OK; }    // the last all-pairs pass's stage 2a read the clamped image: 1, else 0
    if (!std::strcmp(name, "label_order"))      { *value = label_order(c) ? 1 : 0; return SELHIP_OK; }
    if (!std::strcmp(name, "join_tile_rows"))   { *value = join_tile_rows(c); return SELHIP_OK; }
    if (!std::strcmp(name, "join_form_used"))   { *value = c->join_form_used; return SELHIP_OK; }      // kernel FORM of the last LDS-tile join (3 = bit-sliced)
    if (!std::strcmp(name, "chunks"))           { *value = c->n_chunks_last; return SELHIP_OK; }
    if (!std::strcmp(name, "dense_route_used")) { *value = c->dense_route_used; return SELHIP_OK; }         // SELHIP_CRIT_NONE: 1 fused kernel, 0 list route, -1 none yet
    if (!std::strcmp(name, "smhc_path_used"))   { *value = c->smhc_path_used; return SELHIP_OK; }           // SELHIP_CRIT_SMH_C: 1 fast kernel, 0 generic, -1 none yet
    if (!std::strcmp(name, "smhc_rule_used"))   { *value = c->smhc_rule_used; return SELHIP_OK; }           // its threshold rule: 0 fixed c_min, 1 containment, -1 none yet
    if (!std::strcmp(name, "matrix_mirror"))    { *value = c->matrix_mirror; return SELHIP_OK; }
    if (!std::strcmp(name, "matrix_smh_form"))  { *value = c->matrix_smh_form; return SELHIP_OK; }
    if (!std::strcmp(name, "matrix_smh_path_used")) { *value = c->matrix_smh_path_used; return SELHIP_OK; }   // kernel of the last SuperMinHash matrix: 1 fast, 0 generic
    if (!std::strcmp(name, "clusters_last"))    { *value = c->clusters_last; return SELHIP_OK; }            // clusters of the last selhip_ctx_cluster call, -1 = none yet
    if (!std::strcmp(name, "cluster_blocks"))   { *value = g_cluster_blocks.load(std::memory_order_relaxed); return SELHIP_OK; }
    if (!std::strcmp(name, "vertex_blocks"))    { *value = g_vertex_blocks.load(std::memory_order_relaxed); return SELHIP_OK; }
    if (!std::strcmp(name, "greedy_clusters_last")) { *value = c->greedy_clusters_last; return SELHIP_OK; }  // clusters of the last selhip_ctx_cluster_greedy call, -1 = none yet
    if (!std::strcmp(name, "greedy_rounds_last"))   { *value = c->greedy_rounds_last; return SELHIP_OK; }    // ... and the rounds its selection took
    if (!std::strcmp(name, "forest_rounds_last"))   { *value = c->forest_rounds_last; return SELHIP_OK; }    // rounds of the last selhip_ctx_spanning_forest call, -1 = none yet
    if (!std::strcmp(name, "linkage_rounds_last"))  { *value = c->linkage_rounds_last; return SELHIP_OK; }   // rounds of the last selhip_ctx_linkage call, -1 = none yet
    if (!std::strcmp(name, "linkage_merges_last"))  { *value = c->linkage_merges_last; return SELHIP_OK; }   // ... its merges F,
    if (!std::strcmp(name, "linkage_rowscans_last")) { *value = c->linkage_rowscans_last; return SELHIP_OK; } // ... the rows it scanned
    if (!std::strcmp(name, "linkage_rescans_last")) { *value = c->linkage_rescans_last; return SELHIP_OK; }  // ... and its rescan rounds
    if (!std::strcmp(name, "forest_edges_last"))    { *value = c->forest_edges_last; return SELHIP_OK; }     // ... and the edges of its forest
    if (!std::strcmp(name, "small_pass_used"))  { *value = c->small_used ? 1 : 0; return SELHIP_OK; }
    if (!std::strcmp(name, "pairs_route_used")) { *value = c->pairs_route_used; return SELHIP_OK; }         // list passes: 1 signature, 0 direct, 2 no smh_a stage, -1 none yet
    if (!std::strcmp(name, "pairs_gpw"))        { *value = c->pairs_gpw_used; return SELHIP_OK; }           // ... its groups of four entries per wave and batch (0: one lane per entry)
    if (!std::strcmp(name, "pairs_grid"))       { *value = c->pairs_grid_used; return SELHIP_OK; }          // ... and the blocks of its stage-1 kernel
    if (!std::strcmp(name, "query_topk"))       { *value = c->query_topk; return SELHIP_OK; }              // K of the query passes' top-k, 0 = off
    if (!std::strcmp(name, "allpairs_topk"))    { *value = c->allpairs_topk; return SELHIP_OK; }           // K of the all-pairs passes' top-k, 0 = off
    if (!std::strcmp(name, "topk_rounds"))      { *value = (int)std::min<int64_t>(c->topk_rounds, 0x7FFFFFFF); return SELHIP_OK; }   // selhip_ctx_set_topk_rounds: rows per round, 0 = off, -1 = automatic
    if (!std::strcmp(name, "topk_rounds_used")) { *value = c->rounds_used; return SELHIP_OK; }             // rounds of the last all-pairs pass (0: it ran in one)
    if (!std::strcmp(name, "topk_admitted_lo")) { *value = (int)(c->rounds_admitted & 0x7FFFFFFFull); return SELHIP_OK; }            // records its rounds admitted: low ...
    if (!std::strcmp(name, "topk_admitted_hi")) { *value = (int)((c->rounds_admitted >> 31) & 0x7FFFFFFFull); return SELHIP_OK; }    // ... and high 31 bits
    if (!std::strcmp(name, "query_topk_lds_cap")) { *value = kTopkLdsCap; return SELHIP_OK; }              // longest segment its select kernel stages in LDS
    if (!std::strcmp(name, "query_db_sig_builds")) { *value = c->q.db_sig_builds; return SELHIP_OK; }   // database signature builds of the query passes
    if (!std::strcmp(name, "query_db_index_builds")) { *value = c->q.db_idx_builds; return SELHIP_OK; } // builds of ALGO_INDEX's sorted signature index
    if (!std::strcmp(name, "query_db_index_kib")) {                                                     // its resident size (0 = none held)
        const auto& q = c->q;
        const long long words = !q.db_idx_key ? 0 : (2ll * c->n + query_index_dir_stride(q.db_idx_dir_bits)) * q.db_idx_bands;
        *value = (int)std::min<long long>(0x7FFFFFFF, (words * 4 + 1023) / 1024);
        return SELHIP_OK;
    }
    return SELHIP_E_BADARG;
}

int selhip_ctx_set_candidate_begin(selhip_ctx* c, int64_t k_min) {
    if (!c) return SELHIP_E_BADARG;
    if (k_min < 0 || k_min > c->n) { set_err(&c->err, "candidate_begin %lld outside [0, n]", (long long)k_min); return SELHIP_E_BADARG; }
    c->cand_begin = k_min;
    return SELHIP_OK;
}

int selhip_ctx_set_stage2_grouping(selhip_ctx* c, int enable) {
    if (!c) return SELHIP_E_BADARG;
    c->group_stage2 = enable != 0;
    return SELHIP_OK;
}

int selhip_ctx_set_pipeline(selhip_ctx* c, int chunks) {
    if (!c || chunks < -1 || chunks > kMaxChunks) return SELHIP_E_BADARG;
    c->pipeline = chunks;
    return SELHIP_OK;
}

int selhip_ctx_set_criterion(selhip_ctx* c, int criterion) {
    if (!c || criterion < SELHIP_CRIT_SMH_A || criterion > SELHIP_CRIT_SMH_C) return SELHIP_E_BADARG;
    c->criterion = criterion;
    return SELHIP_OK;
}

int selhip_ctx_set_measure(selhip_ctx* c, int measure) {
    if (!c) return SELHIP_E_BADARG;
    if (measure != SELHIP_MEASURE_JACCARD && measure != SELHIP_MEASURE_MAX_CONTAINMENT) {
        set_err(&c->err, "the measure of a pass is SELHIP_MEASURE_JACCARD (%d) or SELHIP_MEASURE_MAX_CONTAINMENT (%d) (got %d)",
                SELHIP_MEASURE_JACCARD, SELHIP_MEASURE_MAX_CONTAINMENT, measure);
        return SELHIP_E_BADARG;
    }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->measure = measure;
    return SELHIP_OK;
}

int selhip_ctx_set_estimator(selhip_ctx* c, int estimator) {
    if (!c) return SELHIP_E_BADARG;
    if (estimator != SELHIP_ESTIMATOR_HLL && estimator != SELHIP_ESTIMATOR_SMH) {
        set_err(&c->err, "the estimator of a pass is SELHIP_ESTIMATOR_HLL (%d) or SELHIP_ESTIMATOR_SMH (%d) (got %d)",
                SELHIP_ESTIMATOR_HLL, SELHIP_ESTIMATOR_SMH, estimator);
        return SELHIP_E_BADARG;
    }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->estimator = estimator;
    return SELHIP_OK;
}

double selhip_smh_value(int measure, int m, int c, uint64_t e1, uint64_t e2) { return selhip::smh_value(measure, m, c, e1, e2); }

int selhip_ctx_set_min_matches(selhip_ctx* c, int c_min) {
    if (!c) return SELHIP_E_BADARG;
    if (c_min < 1) { set_err(&c->err, "min_matches must be >= 1 (got %d)", c_min); return SELHIP_E_BADARG; }
    c->min_matches = c_min;
    return SELHIP_OK;
}

int selhip_ctx_set_min_containment(selhip_ctx* c, double gamma) {
    if (!c) return SELHIP_E_BADARG;
    if (std::isinf(gamma)) { set_err(&c->err, "min_containment must be finite, or NaN to clear it (got %g)", gamma); return SELHIP_E_BADARG; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->min_containment = gamma;                    // (NaN: the fixed rule again)
    return SELHIP_OK;
}

int selhip_smhc_threshold(int m, double gamma, uint64_t e_lo, uint64_t e_hi) { return selhip::smhc_threshold(m, gamma, e_lo, e_hi); }

// the auxiliary HLL registers [n][1 << p_aux] of a sketch set from the host into the set's own buffer (the arguments were checked)
static int upload_aux_hll_rows(selhip_ctx* c, const uint8_t* h_aux_hll, int64_t n, int p_aux, DevBuf<uint8_t>& own, const uint8_t** d_aux_hll, int* p_set) {
    const size_t bytes = (size_t)n << p_aux;
    HIPCHK(&c->err, own.ensure(bytes ? bytes : 1));
    if (bytes) HIPCHK(&c->err, hipMemcpyAsync(own.p, h_aux_hll, bytes, hipMemcpyHostToDevice, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    *d_aux_hll = own.p; *p_set = p_aux;
    return SELHIP_OK;
}

int selhip_ctx_upload_aux_hll(selhip_ctx* c, const uint8_t* h_aux_hll, int p_aux) {
    if (!c || !h_aux_hll || p_aux < 4 || p_aux > kMaxAuxP) return SELHIP_E_BADARG;     // (aux_fused_kernel's bins are 16 bits wide)
    if (!c->d_hll && c->n) { set_err(&c->err, "upload the primary sketches first"); return SELHIP_E_STATE; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    return upload_aux_hll_rows(c, h_aux_hll, c->n, p_aux, c->own_aux_hll, &c->d_aux_hll, &c->p_aux);
}

int selhip_ctx_attach_aux_hll(selhip_ctx* c, const uint8_t* d_aux_hll, int p_aux) {
    if (!c || !d_aux_hll || p_aux < 4 || p_aux > kMaxAuxP) return SELHIP_E_BADARG;
    c->d_aux_hll = d_aux_hll; c->p_aux = p_aux;
    return SELHIP_OK;
}

// the same registers folded on the device from the set's main sketches d_hll [n][1 << c->p] (hll_fold_kernel): leaves what
// upload_aux_hll_rows leaves (the arguments were checked)
static int fold_aux_hll_rows(selhip_ctx* c, const uint8_t* d_hll, int64_t n, int p_aux, DevBuf<uint8_t>& own, const uint8_t** d_aux_hll, int* p_set) {
    const size_t bytes = (size_t)n << p_aux;
    HIPCHK(&c->err, own.ensure(bytes ? bytes : 1));
    if (bytes) HIPCHK(&c->err, launch_hll_fold(c->stream, d_hll, (u64)n, c->p, p_aux, own.p));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    *d_aux_hll = own.p; *p_set = p_aux;
    return SELHIP_OK;
}

// range of a fold's p_aux against the main sketches' precision, with a message
static int check_fold_p(selhip_ctx* c, int p_aux) {
    const int hi = std::min(c->p, kMaxAuxP);
    if (p_aux < 4 || p_aux > hi) { set_err(&c->err, "fold: p_aux %d out of range [4,%d] (p_hll = %d)", p_aux, hi, c->p); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

int selhip_ctx_fold_aux_hll(selhip_ctx* c, int p_aux) {
    if (!c) return SELHIP_E_BADARG;
    if (c->m <= 0 || (!c->d_hll && c->n)) { set_err(&c->err, "upload or attach the primary sketches before folding them"); return SELHIP_E_STATE; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    const int rc = check_fold_p(c, p_aux);
    if (rc) return rc;
    HIPCHK(&c->err, hipSetDevice(c->device));
    return fold_aux_hll_rows(c, c->d_hll, c->n, p_aux, c->own_aux_hll, &c->d_aux_hll, &c->p_aux);
}

static int validate_shape(selhip_ctx* c, int64_t n, int m, int p) {
    if (n < 0 || n > 0x7FFFFFF0ll) { set_err(&c->err, "n_genomes %lld out of range", (long long)n); return SELHIP_E_BADARG; }
    if (m <= 0) { set_err(&c->err, "m must be > 0"); return SELHIP_E_BADARG; }
    if (p < 4 || p > 20) { set_err(&c->err, "p_hll %d out of range [4,20]", p); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

// host cards of a sketch set (`noun` names it in the messages): finite, in [0, 2^63), ascending.  Touches nothing but the message
static int check_host_cards(selhip_ctx* c, const char* noun, const double* cards, int64_t n) {
    for (int64_t i = 0; i < n; ++i) {
        const double v = cards[i];
        if (!(v >= 0.0) || !(v < 9.2e18)) { set_err(&c->err, "%s[%lld] = %g is not a finite value in [0, 2^63)", noun, (long long)i, v); return SELHIP_E_BADARG; }
        if (i && v < cards[i - 1]) { set_err(&c->err, "%s are not in ascending order at rank %lld", noun, (long long)i); return SELHIP_E_BADARG; }
    }
    return SELHIP_OK;
}

// the cards of a sketch set of n genomes (`noun` names it in the messages): computed with the device estimator from d_hll when none
// are given, else validated (unless the caller ran check_host_cards already) and copied from the host, else the caller's device
// array as it is
static int load_cards(selhip_ctx* c, const char* noun, const uint8_t* d_hll, int64_t n, const double* cards_src, bool cards_on_host,
                      DevBuf<double>& own, const double** d_cards, bool host_cards_checked = false) {
    if (!cards_src) {
        HIPCHK(&c->err, own.ensure((size_t)n));
        const int rc = compute_cards(c, d_hll, n, c->p, own.p);
        if (rc) return rc;
        *d_cards = own.p;
    } else if (cards_on_host) {
        if (!host_cards_checked) { const int rc = check_host_cards(c, noun, cards_src, n); if (rc) return rc; }
        HIPCHK(&c->err, own.ensure((size_t)n));
        HIPCHK(&c->err, hipMemcpyAsync(own.p, cards_src, (size_t)n * sizeof(double), hipMemcpyHostToDevice, c->stream));
        *d_cards = own.p;
    } else {
        *d_cards = cards_src;
    }
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

// the products of the sketches the context was just handed: bit planes, sparse lists, cards (host cards were checked by the caller)
static int after_sketches(selhip_ctx* c, const double* cards_src, bool cards_on_host) {
    c->planes.khi = 0; c->hll_sparse_t = 0; c->hll_image_ok = false;
    if (c->n == 0) return SELHIP_OK;
    if (c->p == 14 && c->hist_algo != 0) {
        // the registers once more as bit planes: what stage 2a reads
        int rc = c->planes.build(&c->err, c->stream, c->d_hll, c->n);
        if (rc) return rc;
        // the rare high registers once more as sparse lists (512 B per genome), whatever "hist_sparse" is now: it may change before a pass
        HIPCHK(&c->err, c->hll_sparse.ensure((size_t)c->n * kBsSparseCap));
        HIPCHK(&c->err, c->hll_sparse_dev_t.ensure(1));
        // ... and, where their threshold is 4, 8 or 12, as the clamped image (8 KiB per genome) that stage 2a then reads in place of the planes
        rc = build_sparse_lists(&c->err, c->stream, c->planes.bs.p, c->n, c->hll_sparse.p, c->hll_sparse_dev_t.p, &c->hll_sparse_t, &c->hll_image, &c->hll_image_ok);
        if (rc) return rc;
    }
    return load_cards(c, "cards", c->d_hll, c->n, cards_src, cards_on_host, c->own_cards, &c->d_cards, true);
}

// A replacement of the database in two steps.  Everything that can refuse the call on its ARGUMENTS has passed when set_database
// runs: it is the first statement that changes the context.  What can still fail from there on is a HIP call (an allocation, a copy,
// a kernel of the plane / list / card builds); the context then holds neither the old set (its buffers may be half overwritten) nor
// the new one, so no_database leaves it holding none: the next pass selects nothing, queries and auxiliary sketches are gone
static void set_database(selhip_ctx* c, int64_t n, int m, int p_hll) {
    c->n = n; c->m = m; c->p = p_hll; c->have_run = false; c->pending = false; c->cand_begin = 0; c->sig_key = 0; c->small_pass_failed = false;
    c->d_aux_hll = nullptr; c->p_aux = 0;
    drop_queries(c);
}

static int no_database(selhip_ctx* c, int rc) {
    c->n = 0; c->d_hll = nullptr; c->d_aux = nullptr; c->d_cards = nullptr; c->owns_sketches = false;
    c->planes.khi = 0; c->hll_sparse_t = 0; c->hll_image_ok = false;
    return rc;
}

static int upload_rows(selhip_ctx* c, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards) {
    const size_t hb = (size_t)1 << c->p;
    if (c->n > 0) {
        HIPCHK(&c->err, c->own_hll.ensure((size_t)c->n * hb));
        HIPCHK(&c->err, c->own_aux.ensure((size_t)c->n * c->m));
        HIPCHK(&c->err, hipMemcpyAsync(c->own_hll.p, h_hll, (size_t)c->n * hb, hipMemcpyHostToDevice, c->stream));
        HIPCHK(&c->err, hipMemcpyAsync(c->own_aux.p, h_aux, (size_t)c->n * c->m * 8, hipMemcpyHostToDevice, c->stream));
    }
    c->d_hll = c->own_hll.p; c->d_aux = (const u64*)c->own_aux.p; c->owns_sketches = true;
    return after_sketches(c, h_cards, true);
}

int selhip_ctx_upload(selhip_ctx* c, const uint8_t* h_hll, const uint64_t* h_aux, const double* h_cards,
                      int64_t n, int m, int p_hll) {
    if (!c) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = validate_shape(c, n, m, p_hll);
    if (rc) return rc;
    if (n > 0 && (!h_hll || !h_aux)) { set_err(&c->err, "null sketch pointer"); return SELHIP_E_BADARG; }
    if (h_cards) { rc = check_host_cards(c, "cards", h_cards, n); if (rc) return rc; }
    set_database(c, n, m, p_hll);
    rc = upload_rows(c, h_hll, h_aux, h_cards);
    return rc ? no_database(c, rc) : SELHIP_OK;
}

int selhip_ctx_attach(selhip_ctx* c, const uint8_t* d_hll, const uint64_t* d_aux, const double* d_cards,
                      int64_t n, int m, int p_hll) {
    if (!c) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = validate_shape(c, n, m, p_hll);
    if (rc) return rc;
    if (n > 0 && (!d_hll || !d_aux)) { set_err(&c->err, "null sketch pointer"); return SELHIP_E_BADARG; }
    if (((uintptr_t)d_hll & 15) || ((uintptr_t)d_aux & 15)) { set_err(&c->err, "sketch pointers must be 16-byte aligned"); return SELHIP_E_BADARG; }
    set_database(c, n, m, p_hll);
    c->d_hll = d_hll; c->d_aux = (const u64*)d_aux; c->owns_sketches = false;
    rc = after_sketches(c, d_cards, false);
    return rc ? no_database(c, rc) : SELHIP_OK;
}

int selhip_hll_cards(selhip_ctx* c, const uint8_t* d_hll, int64_t n, int p, double* d_cards_out) {
    if (!c || !d_hll || !d_cards_out || n < 0 || p < 4 || p > 20) return SELHIP_E_BADARG;
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = compute_cards(c, d_hll, n, p, d_cards_out);
    if (rc) return rc;
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int selhip_ctx_get_cards(selhip_ctx* c, double* h_out) {
    if (!c || !h_out) return SELHIP_E_BADARG;
    if (!c->d_cards && c->n) { set_err(&c->err, "no sketches uploaded"); return SELHIP_E_STATE; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    if (c->n) HIPCHK(&c->err, hipMemcpyAsync(h_out, c->d_cards, (size_t)c->n * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    return SELHIP_OK;
}

int selhip_ctx_run_async(selhip_ctx* c, int mode, int algo, float tau_f, int n_rows, int n_bands,
                         int64_t row_begin, int64_t row_end) {
    if (!c) return SELHIP_E_BADARG;
    { const int rc = accept_measure(c, mode); if (rc) return rc; }
    { const int rc = accept_estimator(c); if (rc) return rc; }
    { const int rc = accept_rounds(c); if (rc) return rc; }
    if (c->criterion == SELHIP_CRIT_SMH_C) { const int rc = accept_count(c); if (rc) return rc; }
    if (!c->d_aux && c->n) { set_err(&c->err, "run before upload/attach"); return SELHIP_E_STATE; }
    if (mode != SELHIP_MODE_SMH && mode != SELHIP_MODE_CB_SMH) { set_err(&c->err, "bad mode %d", mode); return SELHIP_E_BADARG; }
    if (algo != SELHIP_ALGO_AUTO && algo != SELHIP_ALGO_STREAM && algo != SELHIP_ALGO_SIG && algo != SELHIP_ALGO_HASHJOIN) { set_err(&c->err, "bad algo %d", algo); return SELHIP_E_BADARG; }
    if (aux_criterion(c->criterion) && !c->d_aux_hll && c->n) {
        set_err(&c->err, "criterion %d needs auxiliary HLL sketches (selhip_ctx_upload_aux_hll)", c->criterion);
        return SELHIP_E_STATE;
    }
    if (c->criterion == SELHIP_CRIT_NONE) { const int rc = accept_dense(c); if (rc) return rc; }
    const PassPlan plan = pass_plan(c->criterion, algo, c->m, n_rows, n_bands, c->estimator);
    if (plan.smh && !plan.count && (n_rows <= 0 || n_bands <= 0 || (long long)n_rows * n_bands != c->m)) {
        // criteria_sketch.hpp:67-70: the reference prints an error and selects nothing; the ABI reports it
        set_err(&c->err, "n_rows*n_bands (%d*%d) != m (%d)", n_rows, n_bands, c->m);
        return SELHIP_E_BADARG;
    }
    if (row_begin < 0 || row_end > c->n || row_begin > row_end) { set_err(&c->err, "bad row range [%lld,%lld)", (long long)row_begin, (long long)row_end); return SELHIP_E_BADARG; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    c->mode = mode; c->algo = algo; c->tau_f = tau_f; c->n_rows = n_rows; c->n_bands = n_bands; c->plan = plan;
    c->row_begin = row_begin; c->row_end = row_end;
    c->have_run = false; c->last_was_query = false; c->topk_applied = false; c->topk_n = 0; c->list_pass = false;
    c->rd = selhip_ctx::Rounds{}; c->rounds_used = 0; c->rounds_admitted = 0;
    c->hist_image_used = 0;                         // (a pass that launches nothing read no image: not the pass before's report)
    std::memset(&c->last, 0, sizeof c->last);
    if (c->n == 0 || row_begin == row_end) { c->pending = false; c->have_run = true; c->topk_applied = c->allpairs_topk > 0; return SELHIP_OK; }
    if (c->topk_rounds != 0) {
        // row rounds: the first round is enqueued here, selhip_ctx_finish merges it and drives the rest.  Every genome's admission
        // threshold starts at -inf
        c->rd.on = true;
        c->rd.rows = topk_round_rows(c->topk_rounds, c->n, interleave_period(c));
        c->rd.begin = row_begin; c->rd.end = std::min<int64_t>(row_end, row_begin + c->rd.rows);
        HIPCHK(&c->err, c->topk_thr.ensure((size_t)c->n));
        hipLaunchKernelGGL(topk_threshold_kernel, dim3((unsigned)((c->n + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, (const selhip_pair_t*)nullptr, (u64)0,
                           (const u64*)nullptr, (int)c->n, c->allpairs_topk, c->topk_thr.p);
        HIPCHK(&c->err, hipGetLastError());
    }
    size_t surv_cap = std::max<size_t>(c->surv.cap, std::max<size_t>((size_t)1 << 20, (size_t)c->n * 16));
    if (join16_pass(c)) {
        // the 16-bit join passes ~n_bands * 2^-16 of the pairs it compares on to the 32-bit filter: size the lists for that
        // up front (an overflow would only cost one repeated pass)
        const double expect = (double)pair_bound(c->n, (int)row_begin, (int)row_end) / std::max(1, c->il_parts) * n_bands / (c->join_bits == 15 ? 32768.0 : 65536.0);
        surv_cap = std::max(surv_cap, (size_t)std::min(expect * 1.25 + 65536.0, (double)((size_t)1 << 26)));
    }
    if (c->init_cap > 0) surv_cap = std::max<size_t>(c->surv.cap, (size_t)c->init_cap);       // test hook: start small, grow on overflow
    size_t res_cap = std::max<size_t>(c->results.cap, surv_cap);
    int rc = ensure_scratch(c, surv_cap, res_cap);
    if (rc) return rc;
    rc = enqueue_pass(c);
    if (rc) return rc;
    c->pending = true;
    return SELHIP_OK;
}

int selhip_ctx_finish(selhip_ctx* c) {
    if (!c) return SELHIP_E_BADARG;
    if (!c->pending) return c->have_run ? SELHIP_OK : SELHIP_E_STATE;
    HIPCHK(&c->err, hipSetDevice(c->device));
    for (int attempt = 0; attempt < kMaxAttempts; ++attempt) {
        HIPCHK(&c->err, wait_stream(c->stream));
        // block 0 = pass-wide counters; blocks 1..chunks = per-row-chunk list counters (each list slice = cap / chunks)
        PassCounters pc = c->h_pc[0];
        const int chunks = c->n_chunks_last;
        if (c->small_used && pc.n_pre_segmax == kSmallOverflow) {
            // a block of the one-launch small pass met more survivors than its LDS list holds: the regular pass from now on
            c->small_pass_failed = true;
            int rc = ensure_scratch(c, c->surv.cap, c->results.cap);
            if (!rc) rc = enqueue_pass(c);
            if (rc) { c->pending = false; return rc; }
            continue;
        }
        if (pc.unsorted) { c->pending = false; set_err(&c->err, "cards are not in ascending order"); return SELHIP_E_BADARG; }
        if (c->list_pass && pc.n_pre) {
            // (block 0 of a list pass: n_pre = invalid entries, n_pre_segmax = 1 + the index of one of them)
            c->pending = false;
            set_err(&c->err, "the pair list holds %llu invalid entries (x == y, or a rank outside [0, %lld)); entry %llu is one",
                    pc.n_pre, (long long)c->n, pc.n_pre_segmax - 1);
            return SELHIP_E_BADARG;
        }
        bool grow = false;
        size_t surv_cap = c->surv.cap, res_cap = c->results.cap;
        const size_t slice = c->surv.cap / (size_t)chunks;
        for (int k = 1; k <= chunks; ++k) {
            const PassCounters& q = c->h_pc[k];
            pc.n_survivors += q.n_survivors; pc.n_candidates += q.n_candidates; pc.n_aux_in += q.n_aux_in; pc.n_final += q.n_final;
            // the 16-bit join's list is kAppendSegs equal slices: it overflows when its fullest slice does
            const u64 worst = std::max(std::max(std::max(q.n_survivors, q.n_candidates), q.n_pre_segmax * (u64)kAppendSegs), !survivors_final(c->criterion) ? q.n_final : 0);
            if (worst > slice && !c->plan.emit) { surv_cap = std::max(surv_cap, grown(worst) * (size_t)chunks); grow = true; }
            // (n_aux_in is zeroed before every enumeration sub-pass, so what arrives here is the LAST sub-pass's count only: it proves
            //  nothing about the others.  The guarantee is the host-side bound in enqueue_pass -- every sub-pass lists at most
            //  cand.cap - 1024 pairs by construction -- and enum_pairs_kernel never writes past out_cap.)
        }
        if (results_overflowed(pc.n_results, c->results.cap, &res_cap)) grow = true;
        if (!grow) {
            if (c->criterion == SELHIP_CRIT_NONE) dense_stats(&pc);
            if (c->rd.on) {
                // a round of a pass in row rounds is accepted: its counters join the pass's, its records are merged into the carried
                // list C (which the repeats of a round that overflowed never touched) and raise the thresholds; then the next round
                // is enqueued and this loop starts over for it
                selhip_ctx::Rounds& rd = c->rd;
                rd.acc.n_evaluated += pc.n_evaluated; rd.acc.n_survivors += pc.n_survivors; rd.acc.n_candidates += pc.n_candidates;
                rd.acc.n_results += pc.n_final;                                  // |S|: the pairs with V >= tau, admitted or not
                rd.attempts = std::max(rd.attempts, attempt + 1);
                c->rounds_used += 1; c->rounds_admitted += pc.n_results;
                c->last = pc;
                int rc = reduce_topk(c, {c->allpairs_topk, c->n, true, "genome", "genomes", true, rd.n_carry});
                if (rc) { c->pending = false; rd.on = false; return rc; }
                rd.n_carry = (u64)c->topk_n;
                if (rd.end < c->row_end) {
                    rd.begin = rd.end; rd.end = std::min<int64_t>(c->row_end, rd.begin + rd.rows);
                    rc = ensure_scratch(c, c->surv.cap, c->results.cap);
                    if (!rc) rc = enqueue_pass(c);
                    if (rc) { c->pending = false; rd.on = false; return rc; }
                    attempt = -1;
                    continue;
                }
                // behind the last round C is nbr(S, K) of the whole pass: it becomes the result list
                // (copied where it fits -- n K records at most -- so that the result list keeps the capacity the rounds grew it to)
                if (rd.n_carry && rd.n_carry <= c->results.cap)
                    HIPCHK(&c->err, hipMemcpyAsync(c->results.p, c->topk_carry.p, (size_t)rd.n_carry * sizeof(selhip_pair_t), hipMemcpyDeviceToDevice, c->stream));
                else if (rd.n_carry) std::swap(c->results, c->topk_carry);
                c->last = rd.acc; c->pending = false; c->have_run = true; c->last_attempts = rd.attempts;
                c->topk_n = (int64_t)rd.n_carry; c->topk_applied = true; rd.on = false;
                return SELHIP_OK;
            }
            c->last = pc; c->pending = false; c->have_run = true; c->last_attempts = attempt + 1;
            // (event pairs are read lazily -- selhip_ctx_kernel_ms / _timing / destroy -- so that a timed run does not stall the
            // host between passes; a pass records at most ~20 of them)
            if (c->allpairs_topk > 0) {
                // the pass is accepted and n_results known: every genome keeps its K best partners, on the same stream
                const int rc = reduce_topk(c, {c->allpairs_topk, c->n, true, "genome", "genomes"});
                if (rc) { c->have_run = false; return rc; }
                c->topk_applied = true;
            }
            return SELHIP_OK;
        }
        // an output list was too small: counts are exact, so grow once and repeat the pass
        res_cap = std::max(res_cap, surv_cap);
        int rc = ensure_scratch(c, surv_cap, res_cap);
        if (rc) { c->pending = false; c->rd.on = false; return rc; }
        rc = c->list_pass ? enqueue_pairs_pass(c) : enqueue_pass(c);
        if (rc) { c->pending = false; c->rd.on = false; return rc; }
    }
    c->pending = false; c->rd.on = false;
    set_err(&c->err, "output buffers kept overflowing");
    return SELHIP_E_OVERFLOW;
}

int selhip_ctx_set_allpairs_topk(selhip_ctx* c, int k) {
    if (!c) return SELHIP_E_BADARG;
    if (k < 0 || k > SELHIP_TOPK_MAX) { set_err(&c->err, "all-pairs top-k must be 0 (off) or in [1, %d] (got %d)", SELHIP_TOPK_MAX, k); return SELHIP_E_BADARG; }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->allpairs_topk = k;
    return SELHIP_OK;
}

int selhip_ctx_set_topk_rounds(selhip_ctx* c, int64_t rows) {
    if (!c) return SELHIP_E_BADARG;
    if (rows < 0 && rows != SELHIP_TOPK_ROUNDS_AUTO) {
        set_err(&c->err, "top-k rounds: 0 (off), rows per round > 0 or SELHIP_TOPK_ROUNDS_AUTO (%d) (got %lld)", SELHIP_TOPK_ROUNDS_AUTO, (long long)rows);
        return SELHIP_E_BADARG;
    }
    if (c->pending) { set_err(&c->err, "a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    c->topk_rounds = rows;
    return SELHIP_OK;
}

int selhip_ctx_run(selhip_ctx* c, int mode, int algo, float tau_f, int n_rows, int n_bands,
                   int64_t row_begin, int64_t row_end) {
    int rc = selhip_ctx_run_async(c, mode, algo, tau_f, n_rows, n_bands, row_begin, row_end);
    if (rc) return rc;
    return selhip_ctx_finish(c);
}

int selhip_ctx_stats(const selhip_ctx* c, int64_t stats[4]) {
    if (!c || !stats) return SELHIP_E_BADARG;
    if (!c->have_run) return SELHIP_E_STATE;
    stats[0] = (int64_t)c->last.n_evaluated;
    stats[1] = (int64_t)(survivors_final(c->criterion) ? c->last.n_survivors : c->last.n_final);
    stats[2] = (int64_t)c->last.n_results;
    stats[3] = (int64_t)(c->last.n_candidates ? c->last.n_candidates : c->last.n_survivors);
    return SELHIP_OK;
}

int64_t selhip_ctx_result_count(const selhip_ctx* c) {
    if (!c || !c->have_run) return SELHIP_E_STATE;
    return result_records(c);
}

int selhip_ctx_fetch(selhip_ctx* c, selhip_pair_t* h_out, int64_t cap) {
    if (!c || (cap > 0 && !h_out) || cap < 0) return SELHIP_E_BADARG;
    if (!c->have_run) return SELHIP_E_STATE;
    const int64_t cnt = result_records(c);
    if (cnt == 0) return SELHIP_OK;
    HIPCHK(&c->err, hipSetDevice(c->device));
    std::vector<selhip_pair_t> tmp((size_t)cnt);
    HIPCHK(&c->err, hipMemcpyAsync(tmp.data(), c->results.p, (size_t)cnt * sizeof(selhip_pair_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    std::sort(tmp.begin(), tmp.end(), [](const selhip_pair_t& a, const selhip_pair_t& b) {
        return a.i != b.i ? a.i < b.i : a.k < b.k;
    });
    std::memcpy(h_out, tmp.data(), (size_t)std::min(cnt, cap) * sizeof(selhip_pair_t));
    return cnt > cap ? SELHIP_E_OVERFLOW : SELHIP_OK;
}

int selhip_ctx_result_device(selhip_ctx* c, const selhip_pair_t** d_results, int64_t* count) {
    if (!c || !d_results || !count) return SELHIP_E_BADARG;
    if (!c->have_run) return SELHIP_E_STATE;
    *d_results = c->results.p;
    *count = result_records(c);
    return SELHIP_OK;
}

int selhip_ctx_copy_results(selhip_ctx* c, selhip_pair_t* d_dst, int64_t cap) {
    if (!c || cap < 0 || (cap > 0 && !d_dst)) return SELHIP_E_BADARG;
    if (!c->have_run) return SELHIP_E_STATE;
    const int64_t cnt = std::min<int64_t>(result_records(c), cap);
    if (cnt > 0) {
        HIPCHK(&c->err, hipSetDevice(c->device));
        HIPCHK(&c->err, hipMemcpyAsync(d_dst, c->results.p, (size_t)cnt * sizeof(selhip_pair_t), hipMemcpyDeviceToDevice, c->stream));
    }
    return SELHIP_OK;
}

int selhip_ctx_copy_results_framed(selhip_ctx* c, void* d_dst, int64_t cap_records) {
    // frame = one 16-byte header record {u64 count, u64 0} followed by the records; both copies are device-to-device
    if (!c || !d_dst || cap_records < 0) return SELHIP_E_BADARG;
    if (!c->have_run) return SELHIP_E_STATE;
    if (c->last_was_query) { set_err(&c->err, "framed copies are for all-pairs passes; after a query pass use selhip_ctx_copy_results"); return SELHIP_E_STATE; }
    if (c->allpairs_topk > 0) { set_err(&c->err, "framed copies carry the pass's own count; with the all-pairs top-k on (selhip_ctx_set_allpairs_topk) use selhip_ctx_copy_results"); return SELHIP_E_STATE; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    HIPCHK(&c->err, hipMemcpyAsync(d_dst, &c->pcb->n_results, sizeof(u64), hipMemcpyDeviceToDevice, c->stream));
    const int64_t cnt = std::min<int64_t>((int64_t)c->last.n_results, cap_records);
    if (cnt > 0)
        HIPCHK(&c->err, hipMemcpyAsync((char*)d_dst + sizeof(selhip_pair_t), c->results.p, (size_t)cnt * sizeof(selhip_pair_t),
                                       hipMemcpyDeviceToDevice, c->stream));
    return (int64_t)c->last.n_results > cap_records ? SELHIP_E_OVERFLOW : SELHIP_OK;
}

int selhip_ctx_copy_results_framed_async(selhip_ctx* c, void* d_dst, int64_t cap_records) {
    if (!c || !d_dst || cap_records < 0) return SELHIP_E_BADARG;
    if (!c->pending && !c->have_run) return SELHIP_E_STATE;
    if (!c->results.p || !c->pcb) return SELHIP_E_STATE;
    if (c->last_was_query && !c->pending) { set_err(&c->err, "framed copies are for all-pairs passes; after a query pass use selhip_ctx_copy_results"); return SELHIP_E_STATE; }
    if (c->allpairs_topk > 0) { set_err(&c->err, "framed copies carry the pass's own count; with the all-pairs top-k on (selhip_ctx_set_allpairs_topk) use selhip_ctx_copy_results"); return SELHIP_E_STATE; }
    HIPCHK(&c->err, hipSetDevice(c->device));
    if ((uintptr_t)d_dst & 15) { set_err(&c->err, "frame buffer must be 16-byte aligned"); return SELHIP_E_BADARG; }
    static_assert(sizeof(selhip_pair_t) == 16, "frame records are 16 bytes");
    hipLaunchKernelGGL(frame_results_kernel, dim3(256), dim3(kBlock), 0, c->stream, c->results.p, &c->pcb->n_results,
                       (u64)c->results.cap, (u64)cap_records, (uint4*)d_dst);
    HIPCHK(&c->err, hipGetLastError());
    return SELHIP_OK;
}

int selhip_ctx_last_attempts(const selhip_ctx* c) { return c ? c->last_attempts : SELHIP_E_BADARG; }

int selhip_ctx_timing(selhip_ctx* c, int enable) {
    if (!c) return SELHIP_E_BADARG;
    (void)hipStreamSynchronize(c->stream);
    drain_timers(c);
    for (int t = 0; t < T_COUNT; ++t) { c->timers[t].total_ms = 0; c->timers[t].launches = 0; c->timers[t].span_ms = 0; }
    c->timing = enable == 2 ? 2 : (enable != 0 ? 1 : 0);
    c->timed_passes = 0;
    for (long& calls : c->timed_calls) calls = 0;
    return SELHIP_OK;
}

static long timed_divisor(const selhip_ctx* c, int t) { return t >= T_MATRIX ? c->timed_calls[t] : c->timed_passes; }   // a call timer's (TimedCall) calls, every other's passes
double selhip_ctx_kernel_ms(const selhip_ctx* c, const char* name) {
    if (!c || !name) return -1.0;
    if (!c->pending) drain_timers(const_cast<selhip_ctx*>(c));
    for (int t = 0; t < T_COUNT; ++t)
        if (!std::strcmp(name, kTimerNames[t])) {
            const long passes = timed_divisor(c, t);
            return (c->timers[t].launches && passes) ? c->timers[t].total_ms / (double)passes : -1.0;
        }
    const long passes = c->timed_passes;
    if (!std::strcmp(name, "join_span"))
        return (c->timers[T_JOIN].launches && passes) ? c->timers[T_JOIN].span_ms / (double)passes : -1.0;
    return -1.0;
}

double selhip_ctx_kernel_launches(const selhip_ctx* c, const char* name) {
    if (!c || !name) return -1.0;
    if (!c->pending) drain_timers(const_cast<selhip_ctx*>(c));
    for (int t = 0; t < T_COUNT; ++t)
        if (!std::strcmp(name, kTimerNames[t])) {
            const long passes = timed_divisor(c, t);
            return passes ? (double)c->timers[t].launches / (double)passes : 0.0;
        }
    return -1.0;
}

}  // extern "C"

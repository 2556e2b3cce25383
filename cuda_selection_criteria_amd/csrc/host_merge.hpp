// host_merge.hpp -- host side of the merge by group (kernel_merge.cuh): the checks, the levels and the launches behind
// selhip_merge_sketches and selhip_ctx_merge_groups, and the scratch either owns.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_greedy.hpp); not a stand-alone header.
#pragma once

namespace {

struct MergeKind { const void* in; void* out; size_t row_bytes; int op; };

// one sketch kind of selhip_merge_sketches: present with both pointers, absent with neither
int merge_check_kind(const char* what, const void* in, const void* out, unsigned align, bool* present) {
    if (!in != !out) { set_err(nullptr, "selhip_merge_sketches: %s: input and output must both be given or both be NULL", what); return SELHIP_E_BADARG; }
    if (((uintptr_t)in | (uintptr_t)out) & (align - 1)) { set_err(nullptr, "selhip_merge_sketches: %s pointers must be %u-byte aligned", what, align); return SELHIP_E_BADARG; }
    *present = in != nullptr;
    return SELHIP_OK;
}

hipError_t merge_scan(hipStream_t st, MergeScratch& ms, int level, size_t slots) {
    size_t bytes = ms.tmp.cap;
    return rocprim::exclusive_scan(ms.tmp.p, bytes, ms.pk.p, ms.scan[level].p, 0ull, slots, rocprim::plus<u64>(), st);
}

// The whole merge on st, behind the argument checks: n members (ids in d_group), G > 0 groups, nk sketch kinds.  Waits for the stream.
// An id outside [-1, G): *bad_out tells, nothing of the caller's is written, SELHIP_OK is returned (the caller words the message).
int merge_run(std::string* err, hipStream_t st, MergeScratch& ms, const MergeKind* kinds, int nk, int64_t n, const int32_t* d_group, int64_t G,
              int32_t* d_size_out, MergeInfo* bad_out) {
    const size_t slots = (size_t)G + 1;
    const unsigned ggrid = (unsigned)((slots + kBlock - 1) / kBlock);
    HIPCHK(err, ms.cnt.ensure((size_t)G));
    HIPCHK(err, ms.order.ensure((size_t)std::max<int64_t>(n, 1)));
    HIPCHK(err, ms.pk.ensure(slots));
    HIPCHK(err, ms.scan[0].ensure(slots));
    HIPCHK(err, ms.info.ensure(1));
    size_t tmp_bytes = 0;
    HIPCHK(err, rocprim::exclusive_scan(nullptr, tmp_bytes, ms.pk.p, ms.scan[0].p, 0ull, slots, rocprim::plus<u64>(), st));
    HIPCHK(err, ms.tmp.ensure(tmp_bytes + 256));

    // level 0: members per group, the check of the ids, offsets
    if (G > 0) HIPCHK(err, hipMemsetAsync(ms.cnt.p, 0, (size_t)G * sizeof(int), st));
    HIPCHK(err, hipMemsetAsync(ms.info.p, 0, sizeof(MergeInfo), st));
    const unsigned ngrid = cluster_vertex_grid(n);                             // (so the "vertex_blocks" hook shapes the two row kernels too)
    if (n > 0) {
        hipLaunchKernelGGL(merge_count_kernel, dim3(ngrid), dim3(kBlock), 0, st, d_group, (long long)n, (int)G, ms.cnt.p, ms.info.p);
        HIPCHK(err, hipGetLastError());
    }
    hipLaunchKernelGGL(merge_pack_kernel, dim3(ggrid), dim3(kBlock), 0, st, ms.cnt.p, (const u64*)nullptr, (int)G, ms.pk.p, ms.info.p);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, merge_scan(st, ms, 0, slots));
    u64 total = 0;
    HIPCHK(err, hipMemcpyAsync(bad_out, ms.info.p, sizeof(MergeInfo), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipMemcpyAsync(&total, ms.scan[0].p + G, sizeof(u64), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    if (bad_out->bad_count) return SELHIP_OK;

    // the levels: while the fullest group has more than S rows, its output rows are partial rows and the members of one more level
    u64 out_rows[kMergeMaxLevels];
    int levels = 1;
    out_rows[0] = (uint32_t)total;
    for (u64 fullest = bad_out->max_cnt; fullest > (u64)kMergeSegment; ++levels) {
        fullest = (fullest + kMergeSegment - 1) / kMergeSegment;
        HIPCHK(err, ms.scan[levels].ensure(slots));
        hipLaunchKernelGGL(merge_pack_kernel, dim3(ggrid), dim3(kBlock), 0, st, (const int*)nullptr, ms.scan[levels - 1].p, (int)G, ms.pk.p, ms.info.p);
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, merge_scan(st, ms, levels, slots));
        HIPCHK(err, hipMemcpyAsync(&total, ms.scan[levels].p + G, sizeof(u64), hipMemcpyDeviceToHost, st));
        HIPCHK(err, hipStreamSynchronize(st));
        out_rows[levels] = (uint32_t)total;
    }
    if (out_rows[levels - 1] != (u64)G) { set_err(err, "merge: %d levels end in %llu rows for %lld groups (internal error)", levels, out_rows[levels - 1], (long long)G); return SELHIP_E_HIP; }
    size_t row_max = 0;
    for (int k = 0; k < nk; ++k) row_max = std::max(row_max, kinds[k].row_bytes);
    for (int l = 0; l + 1 < levels && l < 2; ++l) HIPCHK(err, ms.part[l].ensure((size_t)(out_rows[l] * row_max + 15) / 16));

    if (d_size_out && G > 0) HIPCHK(err, hipMemcpyAsync(d_size_out, ms.cnt.p, (size_t)G * sizeof(int), hipMemcpyDeviceToDevice, st));
    if (n > 0 && G > 0) {
        hipLaunchKernelGGL(merge_scatter_kernel, dim3(ngrid), dim3(kBlock), 0, st, d_group, (long long)n, (int)G, ms.cnt.p, ms.scan[0].p, ms.order.p);
        HIPCHK(err, hipGetLastError());
    }
    for (int k = 0; k < nk; ++k) {
        const void* in = kinds[k].in;
        const int* order = ms.order.p;
        for (int l = 0; l < levels; ++l) {
            void* dst = l + 1 == levels ? kinds[k].out : (void*)ms.part[l & 1].p;
            HIPCHK(err, launch_merge_reduce(st, kinds[k].op, in, order, ms.scan[l].p, (int)G, out_rows[l], out_rows[l] == (u64)G, kinds[k].row_bytes, dst));
            in = dst;
            order = nullptr;
        }
    }
    HIPCHK(err, hipStreamSynchronize(st));
    return SELHIP_OK;
}

void merge_bad_message(std::string* err, const char* who, const MergeInfo& bad, int64_t G) {
    set_err(err, "%s: the group array holds %llu invalid entries (an id outside [-1, %lld)); entry %llu is one", who, bad.bad_count, (long long)G,
            ~bad.bad_index_inv);
}

int merge_sketches_call(const uint8_t* d_hll, const uint64_t* d_smh, const uint8_t* d_aux_hll, int64_t n, int p, int m, int p_aux, const int32_t* d_group,
                        int64_t G, uint8_t* d_hll_out, uint64_t* d_smh_out, uint8_t* d_aux_out, int32_t* d_size_out, hipStream_t st) {
    bool has_hll = false, has_smh = false, has_aux = false;
    int rc = merge_check_kind("hll", d_hll, d_hll_out, 16, &has_hll);
    if (!rc) rc = merge_check_kind("smh", d_smh, d_smh_out, 8, &has_smh);
    if (!rc) rc = merge_check_kind("aux_hll", d_aux_hll, d_aux_out, 16, &has_aux);
    if (rc) return rc;
    if (n < 0 || G < 0 || n > 0x7FFFFFFFll || G > 0x7FFFFFFFll) { set_err(nullptr, "selhip_merge_sketches: 0 <= n, n_groups <= 2^31 - 1"); return SELHIP_E_BADARG; }
    if (p < 4 || p > 20) { set_err(nullptr, "selhip_merge_sketches: p %d out of range [4,20]", p); return SELHIP_E_BADARG; }
    if (has_smh && m <= 0) { set_err(nullptr, "selhip_merge_sketches: m must be > 0 with SuperMinHash rows"); return SELHIP_E_BADARG; }
    if (has_aux && (p_aux < 4 || p_aux > 20)) { set_err(nullptr, "selhip_merge_sketches: p_aux %d out of range [4,20]", p_aux); return SELHIP_E_BADARG; }
    if (n > 0 && !d_group) { set_err(nullptr, "selhip_merge_sketches: null group array"); return SELHIP_E_BADARG; }
    if (((uintptr_t)d_group | (uintptr_t)d_size_out) & 3) { set_err(nullptr, "selhip_merge_sketches: group and size arrays must be 4-byte aligned"); return SELHIP_E_BADARG; }
    if (G == 0 && n == 0) return SELHIP_OK;                                    // (G == 0 with members: every id but -1 is invalid, the count kernel tells)
    MergeKind kinds[3];
    int nk = 0;
    if (has_hll) kinds[nk++] = MergeKind{d_hll, d_hll_out, (size_t)1 << p, kMergeMaxU8};
    if (has_smh) kinds[nk++] = MergeKind{d_smh, d_smh_out, (size_t)m * 8, kMergeMinU64};
    if (has_aux) kinds[nk++] = MergeKind{d_aux_hll, d_aux_out, (size_t)1 << p_aux, kMergeMaxU8};
    MergeScratch ms;
    MergeInfo bad{};
    rc = merge_run(nullptr, st, ms, kinds, G > 0 ? nk : 0, n, d_group, G, d_size_out, &bad);
    ms.release();
    if (rc) return rc;
    if (bad.bad_count) { merge_bad_message(nullptr, "selhip_merge_sketches", bad, G); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

void release_merge(selhip_ctx* c) { c->mg.release(); c->mg_hll.release(); }

int merge_groups_call(selhip_ctx* c, const int32_t* d_group, int64_t G, const selhip_merged_t* out) {
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "selhip_ctx_merge_groups: a pass is still pending (selhip_ctx_finish)"); return SELHIP_E_STATE; }
    if (c->m <= 0 || (c->n && (!c->d_hll || !c->d_aux))) { set_err(&c->err, "selhip_ctx_merge_groups: the context holds no sketches (upload or attach them first)"); return SELHIP_E_STATE; }
    if (!out) { set_err(&c->err, "selhip_ctx_merge_groups: null selhip_merged_t (its members may be null, the struct may not)"); return SELHIP_E_BADARG; }
    if (out->d_aux_hll && !c->d_aux_hll) { set_err(&c->err, "selhip_ctx_merge_groups: d_aux_hll given, but the context holds no auxiliary sketches"); return SELHIP_E_STATE; }
    const int64_t n = c->n;
    if (G < 0 || G > 0x7FFFFFFFll || n > 0x7FFFFFFFll) { set_err(&c->err, "selhip_ctx_merge_groups: 0 <= n_groups <= 2^31 - 1"); return SELHIP_E_BADARG; }
    if (n > 0 && !d_group) { set_err(&c->err, "selhip_ctx_merge_groups: null group array"); return SELHIP_E_BADARG; }
    if (((uintptr_t)out->d_hll | (uintptr_t)out->d_aux_hll) & 15) { set_err(&c->err, "selhip_ctx_merge_groups: d_hll and d_aux_hll must be 16-byte aligned"); return SELHIP_E_BADARG; }
    if (((uintptr_t)out->d_aux | (uintptr_t)out->d_cards) & 7) { set_err(&c->err, "selhip_ctx_merge_groups: d_aux and d_cards must be 8-byte aligned"); return SELHIP_E_BADARG; }
    if (((uintptr_t)d_group | (uintptr_t)out->d_size) & 3) { set_err(&c->err, "selhip_ctx_merge_groups: the group and size arrays must be 4-byte aligned"); return SELHIP_E_BADARG; }
    if (G == 0 && n == 0) return SELHIP_OK;
    HIPCHK(&c->err, hipSetDevice(c->device));
    // the cardinalities are those of the merged main registers: without d_hll they are merged into scratch
    uint8_t* hll_out = out->d_hll;
    if (!hll_out && out->d_cards && G > 0) {
        HIPCHK(&c->err, c->mg_hll.ensure((size_t)G << c->p));
        hll_out = c->mg_hll.p;
    }
    MergeKind kinds[3];
    int nk = 0;
    if (hll_out) kinds[nk++] = MergeKind{c->d_hll, hll_out, (size_t)1 << c->p, kMergeMaxU8};
    if (out->d_aux) kinds[nk++] = MergeKind{c->d_aux, out->d_aux, (size_t)c->m * 8, kMergeMinU64};
    if (out->d_aux_hll) kinds[nk++] = MergeKind{c->d_aux_hll, out->d_aux_hll, (size_t)1 << c->p_aux, kMergeMaxU8};
    // timed as "merge", per merge call: a counter of its own, like "cluster" (level 2 keeps these launches' events)
    MergeInfo bad{};
    int rc;
    {
        TimedCall call(c, T_MERGE);
        TimerScope t(c, T_MERGE);
        rc = merge_run(&c->err, c->stream, c->mg, kinds, G > 0 ? nk : 0, n, d_group, G, out->d_size, &bad);
        if (!rc && !bad.bad_count && out->d_cards && G > 0) rc = compute_cards(c, hll_out, G, c->p, out->d_cards);
    }
    if (rc) return rc;
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    if (bad.bad_count) { merge_bad_message(&c->err, "selhip_ctx_merge_groups", bad, G); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

}  // namespace

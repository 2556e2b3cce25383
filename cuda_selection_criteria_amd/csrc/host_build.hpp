// host_build.hpp -- host side of the split sketch builder (selhip_build_sketches_split; kernels in kernel_sketch.cuh, the plan in
// host_plan.hpp): the checks, the work items, the launches, the reduction through merge_run and the fallback launch.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_merge.hpp); not a stand-alone header.
#pragma once

namespace {

size_t sketch_build_smem(int m, int p_aux, bool has_smh, bool has_aux) {                 // as selhip_build_sketches
    const size_t ms = has_smh ? (size_t)m : 0;
    return ms * 8 + 16384 + (has_aux ? ((((size_t)1 << p_aux) + 3) / 4 * 4) : 0) + ms * 12 + 16;
}

hipError_t sketch_items_attr() {
    static std::once_flag once;
    static hipError_t attr_err = hipSuccess;
    std::call_once(once, [] { attr_err = hipFuncSetAttribute((const void*)sketch_build_items_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024); });
    return attr_err;
}

// the block size of a launch of n_items work items: selhip_build_sketches's rule
unsigned sketch_items_threads(int64_t n_items) { return n_items < 2048 ? 1024u : (unsigned)kBlock; }

struct BuildScratch {
    DevBuf<SketchItem> items;
    DevBuf<long long> genome;           // [split genomes] the output row of each
    DevBuf<int> group, fb;              // [chunks] the split genome of every partial row; fb[0] = fallback count, fb[1 ..] = the list
    DevBuf<uint4> hll_part, smh_part, aux_part, hll_merged, smh_merged, aux_merged;
    MergeScratch ms;
    // the host sides of the copies: they live until the caller has waited for the stream
    std::vector<SketchItem> h_items, h_again;
    std::vector<long long> h_genome;
    std::vector<int> h_group, h_fb;
    void release() {
        items.release(); genome.release(); group.release(); fb.release(); hll_part.release(); smh_part.release(); aux_part.release();
        hll_merged.release(); smh_merged.release(); aux_merged.release(); ms.release();
    }
};

struct BuildArgs {
    const uint8_t* d_codes; int k, m, p_aux;
    uint8_t* d_hll; u64* d_smh; uint8_t* d_aux_hll;
};

int launch_sketch_items(hipStream_t st, const BuildArgs& a, const SketchItem* d_items, int64_t n_items, BuildScratch& bs) {
    const size_t smem = sketch_build_smem(a.m, a.p_aux, a.d_smh != nullptr, a.d_aux_hll != nullptr);
    hipLaunchKernelGGL(sketch_build_items_kernel, dim3((unsigned)n_items), dim3(sketch_items_threads(n_items)), smem, st, a.d_codes, d_items, a.k, a.m,
                       a.p_aux, a.d_hll, a.d_smh, a.d_aux_hll, (uint8_t*)bs.hll_part.p, (u64*)bs.smh_part.p, (uint8_t*)bs.aux_part.p);
    HIPCHK(nullptr, hipGetLastError());
    return SELHIP_OK;
}

// The split build on st behind the checks: off are the validated host offsets, plan has a split genome, counts[g] the chunks of genome g.
int build_split_run(hipStream_t st, const BuildArgs& a, const int64_t* off, int64_t n, const SplitPlan& plan, const std::vector<int64_t>& counts,
                    BuildScratch& bs, selhip_build_info_t* info) {
    const long long C = plan.chunk, S = plan.split_genomes, P = plan.chunks;
    const int n_aux = a.d_aux_hll ? 1 << a.p_aux : 0;
    const int ms = a.d_smh ? a.m : 0;

    // the items: partial ones first (uniform and long), then the whole genomes, longest first
    std::vector<SketchItem>& items = bs.h_items;
    std::vector<long long>& genome = bs.h_genome;
    std::vector<int>& group = bs.h_group;
    items.reserve((size_t)plan.items);
    genome.reserve((size_t)S);
    group.reserve((size_t)P);
    for (int64_t g = 0; g < n; ++g) {
        if (counts[g] < 2) continue;
        const long long L = off[g + 1] - off[g];
        for (long long c = 0; c < counts[g]; ++c) {
            items.push_back(SketchItem{off[g] + c * C, std::min<long long>(C + a.k - 1, L - c * C), (long long)group.size(), kSketchItemPartial, 0});
            group.push_back((int)genome.size());
        }
        genome.push_back(g);
    }
    const size_t first_direct = items.size();
    for (int64_t g = 0; g < n; ++g)
        if (counts[g] < 2) items.push_back(SketchItem{off[g], off[g + 1] - off[g], g, kSketchItemDirect, 0});
    std::stable_sort(items.begin() + first_direct, items.end(), [](const SketchItem& x, const SketchItem& y) { return x.len > y.len; });
    if ((long long)items.size() != plan.items || (long long)group.size() != P || (long long)genome.size() != S) {
        set_err(nullptr, "selhip_build_sketches_split: the items do not add up to the plan (internal error)");
        return SELHIP_E_HIP;
    }

    HIPCHK(nullptr, sketch_items_attr());
    HIPCHK(nullptr, bs.items.ensure(items.size()));
    HIPCHK(nullptr, bs.genome.ensure((size_t)S));
    HIPCHK(nullptr, bs.group.ensure((size_t)P));
    HIPCHK(nullptr, bs.fb.ensure((size_t)S + 1));
    HIPCHK(nullptr, bs.hll_part.ensure((size_t)P * (16384 / 16)));
    HIPCHK(nullptr, bs.hll_merged.ensure((size_t)S * (16384 / 16)));
    if (ms) {
        HIPCHK(nullptr, bs.smh_part.ensure(((size_t)P * ms * 8 + 15) / 16));
        HIPCHK(nullptr, bs.smh_merged.ensure(((size_t)S * ms * 8 + 15) / 16));
    }
    if (n_aux) {
        HIPCHK(nullptr, bs.aux_part.ensure((size_t)P * n_aux / 16));
        HIPCHK(nullptr, bs.aux_merged.ensure((size_t)S * n_aux / 16));
    }
    HIPCHK(nullptr, hipMemcpyAsync(bs.items.p, items.data(), items.size() * sizeof(SketchItem), hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hipMemcpyAsync(bs.genome.p, genome.data(), genome.size() * sizeof(long long), hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hipMemcpyAsync(bs.group.p, group.data(), group.size() * sizeof(int), hipMemcpyHostToDevice, st));
    HIPCHK(nullptr, hipMemsetAsync(bs.fb.p, 0, sizeof(int), st));

    int rc = launch_sketch_items(st, a, bs.items.p, (int64_t)items.size(), bs);
    if (rc) return rc;

    // the partial rows of split genome s are the group s of a merge: u8 maximum, u64 minimum, u8 maximum
    MergeKind kinds[3];
    int nk = 0;
    kinds[nk++] = MergeKind{bs.hll_part.p, bs.hll_merged.p, 16384, kMergeMaxU8};
    if (ms) kinds[nk++] = MergeKind{bs.smh_part.p, bs.smh_merged.p, (size_t)ms * 8, kMergeMinU64};
    if (n_aux) kinds[nk++] = MergeKind{bs.aux_part.p, bs.aux_merged.p, (size_t)n_aux, kMergeMaxU8};
    MergeInfo bad{};
    rc = merge_run(nullptr, st, bs.ms, kinds, nk, P, bs.group.p, S, nullptr, &bad);
    if (rc) return rc;
    if (bad.bad_count || (long long)bad.max_cnt != plan.max_chunks) {
        set_err(nullptr, "selhip_build_sketches_split: the reduction saw other groups than the plan's (internal error)");
        return SELHIP_E_HIP;
    }

    const int smh_vec = ms && ms % 2 == 0 && !((uintptr_t)a.d_smh & 15);
    hipLaunchKernelGGL(sketch_split_finish_kernel, dim3((unsigned)S), dim3(kBlock), 0, st, bs.genome.p, a.m, n_aux, smh_vec, bs.hll_merged.p,
                       (const u64*)bs.smh_merged.p, bs.aux_merged.p, a.d_hll, a.d_smh, a.d_aux_hll, bs.fb.p, bs.fb.p + 1);
    HIPCHK(nullptr, hipGetLastError());

    // the fallback: split genomes whose merged buckets say that pass 0 was not final, rebuilt whole (HLL-only calls have none)
    long long n_fb = 0;
    if (ms) {
        std::vector<int>& fb = bs.h_fb;
        fb.assign((size_t)S + 1, 0);
        HIPCHK(nullptr, hipMemcpyAsync(fb.data(), bs.fb.p, fb.size() * sizeof(int), hipMemcpyDeviceToHost, st));
        HIPCHK(nullptr, hipStreamSynchronize(st));
        n_fb = fb[0];
        if (n_fb < 0 || n_fb > S) { set_err(nullptr, "selhip_build_sketches_split: fallback count %lld of %lld split genomes (internal error)", n_fb, S); return SELHIP_E_HIP; }
        if (n_fb > 0) {
            std::vector<SketchItem>& again = bs.h_again;
            for (long long j = 0; j < n_fb; ++j) {
                const int s = fb[1 + j];
                if (s < 0 || s >= S) { set_err(nullptr, "selhip_build_sketches_split: fallback entry %d outside the split genomes (internal error)", s); return SELHIP_E_HIP; }
                const long long g = genome[s];
                again.push_back(SketchItem{off[g], off[g + 1] - off[g], g, kSketchItemDirect, 0});
            }
            std::stable_sort(again.begin(), again.end(), [](const SketchItem& x, const SketchItem& y) { return x.len > y.len; });
            HIPCHK(nullptr, bs.items.ensure(again.size()));
            HIPCHK(nullptr, hipMemcpyAsync(bs.items.p, again.data(), again.size() * sizeof(SketchItem), hipMemcpyHostToDevice, st));
            rc = launch_sketch_items(st, a, bs.items.p, (int64_t)again.size(), bs);
            if (rc) return rc;
        }
    }
    HIPCHK(nullptr, hipStreamSynchronize(st));
    if (info) info->fallback_genomes = n_fb;
    return SELHIP_OK;
}

void build_info_from_plan(const SplitPlan& p, int64_t n, selhip_build_info_t* info) {
    if (!info) return;
    *info = selhip_build_info_t{};
    info->chunk = p.chunk; info->items = p.items; info->split_genomes = p.split_genomes; info->chunks = p.chunks;
    info->levels = split_levels_of(p.max_chunks);
    info->threads = n > 0 ? (int32_t)sketch_items_threads(p.items) : 0;
}

int build_split_plan_call(const int64_t* h_offsets, int64_t n, int k, int m, int p_aux, int64_t chunk, int64_t resident_blocks, int64_t* counts,
                          selhip_build_info_t* info, SplitPlan* plan_out, const char* who) {
    if (n < 0 || (n > 0 && !h_offsets) || k < 1 || k > 32 || m < 0 || p_aux < 0 || p_aux > 20) { set_err(nullptr, "%s: bad argument", who); return SELHIP_E_BADARG; }
    SplitPlan plan;
    switch (split_plan(h_offsets, n, k, m, p_aux, chunk, resident_blocks, counts, &plan)) {
        case kSplitPlanOk: break;
        case kSplitPlanBadChunk:
            set_err(nullptr, "%s: chunk %lld is neither SELHIP_SPLIT_OFF, SELHIP_SPLIT_AUTO nor a positive multiple of %d end positions", who, (long long)chunk, kSketchSeg);
            return SELHIP_E_BADARG;
        case kSplitPlanBadOffsets:
            set_err(nullptr, "%s: the offsets are negative or descend", who);
            return SELHIP_E_BADARG;
        case kSplitPlanScratch:
            set_err(nullptr, "%s: chunk %lld needs more than %llu bytes of partial rows (%llu bytes per chunk); use a longer chunk or SELHIP_SPLIT_AUTO", who,
                    (long long)chunk, kSplitScratchMax, split_row_bytes(m, p_aux));
            return SELHIP_E_NOMEM;
    }
    build_info_from_plan(plan, n, info);
    if (plan_out) *plan_out = plan;
    return SELHIP_OK;
}

int build_sketches_split_call(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n, int k, int m, int p_aux, int64_t chunk,
                              uint8_t* d_hll, uint64_t* d_smh, uint8_t* d_aux_hll, selhip_build_info_t* info, hipStream_t st) {
    const char* who = "selhip_build_sketches_split";
    // the checks of selhip_build_sketches, then the chunk and the alignment of what the finish kernel stores 16 bytes at a time
    if (!d_codes || !d_offsets || !d_hll || n < 0 || k < 1 || k > 32) { set_err(nullptr, "%s: bad argument", who); return SELHIP_E_BADARG; }
    if (d_smh && (!is_pow2(m) || m > 2048)) { set_err(nullptr, "%s: m must be a power of two <= 2048 (SizePow2Policy rounds up: pass the rounded value)", who); return SELHIP_E_BADARG; }
    if (d_aux_hll && (p_aux < 4 || p_aux > 12)) { set_err(nullptr, "%s: p_aux out of range [4,12]", who); return SELHIP_E_BADARG; }
    if (chunk != SELHIP_SPLIT_OFF && chunk != SELHIP_SPLIT_AUTO && (chunk < 0 || chunk % kSketchSeg)) {
        set_err(nullptr, "%s: chunk %lld is neither SELHIP_SPLIT_OFF, SELHIP_SPLIT_AUTO nor a positive multiple of %d end positions", who, (long long)chunk, kSketchSeg);
        return SELHIP_E_BADARG;
    }
    if (chunk != SELHIP_SPLIT_OFF && ((((uintptr_t)d_hll | (uintptr_t)d_aux_hll) & 15) || ((uintptr_t)d_smh & 7))) {
        set_err(nullptr, "%s: d_hll and d_aux_hll must be 16-byte, d_smh 8-byte aligned", who);
        return SELHIP_E_BADARG;
    }
    const int pm = d_smh ? m : 0, pp = d_aux_hll ? p_aux : 0;
    if (info) *info = selhip_build_info_t{};
    if (n == 0) return SELHIP_OK;

    SplitPlan plan;
    std::vector<int64_t> host_off, counts;
    if (chunk == SELHIP_SPLIT_OFF) {
        plan.items = n;
    } else {
        if (!h_offsets) {
            host_off.resize((size_t)n + 1);
            HIPCHK(nullptr, hipMemcpyAsync(host_off.data(), d_offsets, host_off.size() * sizeof(int64_t), hipMemcpyDeviceToHost, st));
            HIPCHK(nullptr, hipStreamSynchronize(st));
            h_offsets = host_off.data();
        }
        int64_t resident = 1;
        if (chunk == SELHIP_SPLIT_AUTO) {
            // B: the workgroups of the items kernel the device holds at once, at this call's LDS size and 1 024 threads
            int dev = 0, cus = 0, per_cu = 0;
            HIPCHK(nullptr, sketch_items_attr());
            HIPCHK(nullptr, hipGetDevice(&dev));
            HIPCHK(nullptr, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev));
            HIPCHK(nullptr, hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, sketch_build_items_kernel, 1024,
                                                                         sketch_build_smem(m, p_aux, d_smh != nullptr, d_aux_hll != nullptr)));
            resident = std::max<int64_t>(1, (int64_t)cus * per_cu);
        }
        counts.resize((size_t)n);
        const int rc = build_split_plan_call(h_offsets, n, k, pm, pp, chunk, resident, counts.data(), nullptr, &plan, who);
        if (rc) return rc;
    }
    build_info_from_plan(plan, n, info);

    if (plan.split_genomes == 0) {                        // the old launch: same grid, block, LDS and arguments
        const int rc = selhip_build_sketches(d_codes, d_offsets, n, k, m, p_aux, d_hll, d_smh, d_aux_hll, (void*)st);
        if (rc) return rc;
        HIPCHK(nullptr, hipStreamSynchronize(st));
        return SELHIP_OK;
    }
    BuildScratch bs;
    const BuildArgs a{d_codes, k, m, p_aux, d_hll, (u64*)d_smh, d_aux_hll};
    const int rc = build_split_run(st, a, h_offsets, n, plan, counts, bs, info);
    if (rc) (void)hipStreamSynchronize(st);               // nothing of the scratch is freed under a running kernel
    bs.release();
    return rc;
}

}  // namespace

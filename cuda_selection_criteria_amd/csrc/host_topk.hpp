// host_topk.hpp -- host side of the query passes' top-k (kernel_topk.cuh): scratch sized from the pass's record count, the four
// launches behind an accepted pass, and which count the result accessors expose.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_query.hpp); not a stand-alone header.
#pragma once

namespace {

void release_topk(selhip_ctx* c) {
    c->topk_cnt.release(); c->topk_off.release(); c->topk_key.release(); c->topk_val.release(); c->topk_tmp.release();
}

// records held by the result list: the reduced count behind a query pass with top-k on, else what the pass selected
int64_t result_records(const selhip_ctx* c) { return c->topk_applied ? c->topk_n : (int64_t)c->last.n_results; }

// Behind an accepted query pass (c->last holds its counters, c->results its n_results records): the result list becomes topk(S, K) in
// ranked order, c->topk_n its length.  The records are regrouped into (key, rank) arrays first, so the select writes the result list
// in place: the grouped arrays are the second buffer.  On an error the caller withdraws the pass (nothing unreduced passes as reduced).
int reduce_query_topk(selhip_ctx* c) {
    const int K = c->query_topk;
    const u64 n = c->last.n_results;
    const int64_t n_q = c->q.n;
    c->topk_n = 0;
    if (n == 0 || n_q <= 0 || c->n == 0) return SELHIP_OK;                  // nothing selected: nothing is launched
    if (n > 0x7FFFFFFFull) {
        set_err(&c->err, "query top-k takes passes of up to 2^31 - 1 selected pairs (this one selected %llu)", n);
        return SELHIP_E_BADARG;
    }
    const size_t slots = (size_t)n_q + 1;                                     // one past the last query: the scan's totals land there
    hipError_t e = c->topk_cnt.ensure(2 * slots);                             // [0, slots) counts, [slots, 2 slots) fill cursors
    if (e == hipSuccess) e = c->topk_off.ensure(slots);
    if (e == hipSuccess) e = c->topk_key.ensure((size_t)n);
    if (e == hipSuccess) e = c->topk_val.ensure((size_t)n);
    const auto packed = rocprim::make_transform_iterator(c->topk_cnt.p, TopkPack{(uint32_t)K});
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream);
    if (e == hipSuccess) e = c->topk_tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "query top-k: scratch for %llu selected pairs of %lld queries: %s", n, (long long)n_q, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    u64 totals = 0;
    {
        TimerScope t(c, T_TOPK);
        const unsigned blocks = grid_for(n, kWavesPerBlock * kTopkTile * kWave, 4096);
        HIPCHK(&c->err, hipMemsetAsync(c->topk_cnt.p, 0, 2 * slots * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(topk_count_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_q, c->topk_cnt.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->topk_tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->topk_tmp.p, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream));
        hipLaunchKernelGGL(topk_scatter_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_q, c->topk_off.p,
                           c->topk_cnt.p + slots, c->topk_key.p, c->topk_val.p);
        HIPCHK(&c->err, hipGetLastError());
        hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)n_q), dim3(kTopkBlock), kTopkLdsBytes, c->stream, c->topk_key.p, c->topk_val.p,
                           c->topk_off.p, K, c->results.p, (u64)c->results.cap);
        HIPCHK(&c->err, hipGetLastError());
    }
    HIPCHK(&c->err, hipMemcpyAsync(&totals, c->topk_off.p + n_q, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(&c->err, hipStreamSynchronize(c->stream));
    if ((uint32_t)totals != (uint32_t)n) {
        set_err(&c->err, "query top-k: %u of %llu records carry a query rank (internal error)", (uint32_t)totals, n);
        return SELHIP_E_HIP;
    }
    c->topk_n = (int64_t)(totals >> 32);
    return SELHIP_OK;
}

}  // namespace

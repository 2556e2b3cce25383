// host_topk.hpp -- host side of the query passes' top-k (kernel_topk.cuh) and of the all-pairs passes' (kernel_nbr.cuh): scratch sized
// from the pass's record count, the four launches behind an accepted pass, and which count the result accessors expose.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_query.hpp); not a stand-alone header.
#pragma once

namespace {

void release_topk(selhip_ctx* c) {
    c->topk_cnt.release(); c->topk_off.release(); c->topk_key.release(); c->topk_val.release(); c->topk_tmp.release();
}

// records held by the result list: the reduced count behind a pass that was cut (a query pass with query_topk on, an all-pairs pass
// with allpairs_topk on), else what the pass selected
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

// Behind an accepted all-pairs pass (c->last holds its counters, c->results its n_results records {i, k, J}, i < k): the result list
// becomes nbr(S, K) -- every genome's K best partners, records {owner, partner, J}, in ranked order -- and c->topk_n its length, which
// may exceed n_results (at most twice).  Every record is regrouped twice, once per member, into the (key, partner) arrays; the pass's own
// records are dead after that scatter, so a result buffer too small for the reduced list is reallocated before the select writes it.
// On an error the caller withdraws the pass.
int reduce_allpairs_topk(selhip_ctx* c) {
    const int K = c->allpairs_topk;
    const u64 n = c->last.n_results;
    const int64_t n_g = c->n;
    c->topk_n = 0;
    if (n == 0 || n_g <= 0) return SELHIP_OK;                                 // nothing selected: nothing is launched
    if (2 * n > 0x7FFFFFFFull) {
        set_err(&c->err, "all-pairs top-k takes passes of up to 2^30 - 1 selected pairs, 2^31 - 1 directed records (this one selected %llu)", n);
        return SELHIP_E_BADARG;
    }
    const u64 n_dir = 2 * n;
    const size_t slots = (size_t)n_g + 1;                                     // one past the last genome: the scan's totals land there
    hipError_t e = c->topk_cnt.ensure(2 * slots);                             // [0, slots) counts, [slots, 2 slots) fill cursors
    if (e == hipSuccess) e = c->topk_off.ensure(slots);
    if (e == hipSuccess) e = c->topk_key.ensure((size_t)n_dir);
    if (e == hipSuccess) e = c->topk_val.ensure((size_t)n_dir);
    const auto packed = rocprim::make_transform_iterator(c->topk_cnt.p, TopkPack{(uint32_t)K});
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream);
    if (e == hipSuccess) e = c->topk_tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "all-pairs top-k: scratch for %llu selected pairs of %lld genomes: %s", n, (long long)n_g, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    u64 totals = 0;
    bool have_totals = false;
    const auto read_totals = [&]() -> int {
        HIPCHK(&c->err, hipMemcpyAsync(&totals, c->topk_off.p + n_g, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(&c->err, hipStreamSynchronize(c->stream));
        if ((uint32_t)totals != (uint32_t)n_dir) {
            set_err(&c->err, "all-pairs top-k: %u of %llu directed records carry a genome rank (internal error)", (uint32_t)totals, n_dir);
            return SELHIP_E_HIP;
        }
        have_totals = true;
        return SELHIP_OK;
    };
    {
        TimerScope t(c, T_TOPK);
        const unsigned blocks = grid_for(n, kWavesPerBlock * kTopkTile * kWave, 4096);
        HIPCHK(&c->err, hipMemsetAsync(c->topk_cnt.p, 0, 2 * slots * sizeof(uint32_t), c->stream));
        hipLaunchKernelGGL(nbr_count_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_g, c->topk_cnt.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->topk_tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->topk_tmp.p, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream));
        hipLaunchKernelGGL(nbr_scatter_kernel, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_g, c->topk_off.p,
                           c->topk_cnt.p + slots, c->topk_key.p, c->topk_val.p, n_dir);
        HIPCHK(&c->err, hipGetLastError());
        // the reduced list holds sum_g min(L_g, K) <= min(2 n, n_g K) records: only where that bound does not fit is the exact count
        // read before the select, and the result buffer grown to it
        if (std::min<u64>(n_dir, (u64)n_g * (u64)K) > (u64)c->results.cap) {
            const int rc = read_totals();
            if (rc) return rc;
            const size_t need = (size_t)(totals >> 32);
            if (need > c->results.cap && (e = c->results.ensure(need)) != hipSuccess) {
                set_err(&c->err, "all-pairs top-k: result list of %zu records: %s", need, hipGetErrorString(e));
                return SELHIP_E_HIP;
            }
        }
        hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)n_g), dim3(kTopkBlock), kTopkLdsBytes, c->stream, c->topk_key.p, c->topk_val.p,
                           c->topk_off.p, K, c->results.p, (u64)c->results.cap);
        HIPCHK(&c->err, hipGetLastError());
    }
    if (!have_totals) { const int rc = read_totals(); if (rc) return rc; }
    c->topk_n = (int64_t)(totals >> 32);
    return SELHIP_OK;
}

}  // namespace

// host_topk.hpp -- host side of the top-k of the query passes and of the all-pairs passes (kernel_topk.cuh): scratch sized from the
// pass's record count, the four launches behind an accepted pass, and which count the result accessors expose.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_query.hpp); not a stand-alone header.
#pragma once

namespace {

void release_topk(selhip_ctx* c) {
    c->topk_cnt.release(); c->topk_off.release(); c->topk_key.release(); c->topk_val.release(); c->topk_tmp.release();
    c->topk_carry.release(); c->topk_thr.release();
}

// records held by the result list: the reduced count behind a pass that was cut (a query pass with query_topk on, an all-pairs pass
// with allpairs_topk on), else what the pass selected
int64_t result_records(const selhip_ctx* c) { return c->topk_applied ? c->topk_n : (int64_t)c->last.n_results; }

// What a pass asks of reduce_topk.  A query pass: every query keeps its K best records, one owner per record.  An all-pairs pass: every
// genome keeps its K best partners, and every record {i, k, J}, i < k, is grouped twice, once per member (both).
struct TopkJob {
    int K;
    int64_t owners;                     // queries / genomes: one segment each
    bool both;
    const char* owner, * owner_pl;      // the messages' nouns
    // a round of a pass in row rounds (selhip_ctx_set_topk_rounds) MERGES: the carried list C = c->topk_carry[0, n_carry) -- directed
    // records {owner, partner, V}, grouped once -- joins the round's records in the same segments, the select writes the new C back
    // into c->topk_carry, and topk_threshold_kernel writes every owner's admission threshold behind it.  The result list is not touched
    bool merge = false;
    u64 n_carry = 0;
};

// Behind an accepted pass (c->last holds its counters, c->results its n_results records): the result list becomes topk(S, K) -- with
// job.both nbr(S, K): records {owner, partner, J} -- in ranked order, c->topk_n its length, which with job.both may exceed n_results
// (at most twice).  The (directed) records are regrouped into (key, partner) arrays first; the pass's own records are dead after that
// scatter, so the select writes the result list in place: the grouped arrays are the second buffer.  On an error the caller withdraws
// the pass (nothing unreduced passes as reduced).
int reduce_topk(selhip_ctx* c, const TopkJob& job) {
    const int K = job.K;
    const u64 n = c->last.n_results, n_dir = (job.both ? 2 * n : n) + job.n_carry;
    const int64_t n_own = job.owners;
    const char* pass = job.both ? "all-pairs" : "query";
    DevBuf<selhip_pair_t>& out = job.merge ? c->topk_carry : c->results;      // where the reduced list goes
    c->topk_n = (int64_t)job.n_carry;
    if (n == 0 || n_own <= 0 || c->n == 0) return SELHIP_OK;                  // nothing selected: nothing is launched (a merge keeps C and the thresholds)
    if (n_dir > 0x7FFFFFFFull) {
        if (job.merge)
            set_err(&c->err, "all-pairs top-k in row rounds takes up to 2^31 - 1 directed records a round (%llu carried + 2 x %llu admitted): "
                             "fewer rows per round (selhip_ctx_set_topk_rounds)", job.n_carry, n);
        else
            set_err(&c->err, "%s top-k takes passes of up to %s (this one selected %llu)%s", pass,
                    job.both ? "2^30 - 1 selected pairs, 2^31 - 1 directed records" : "2^31 - 1 selected pairs", n,
                    job.both ? "; an smh_c pass under the estimator smh runs beyond that in row rounds (selhip_ctx_set_topk_rounds)" : "");
        return SELHIP_E_BADARG;
    }
    c->topk_n = 0;
    const size_t slots = (size_t)n_own + 1;                                   // one past the last owner: the scan's totals land there
    hipError_t e = c->topk_cnt.ensure(2 * slots);                             // [0, slots) counts, [slots, 2 slots) fill cursors
    if (e == hipSuccess) e = c->topk_off.ensure(slots);
    if (e == hipSuccess) e = c->topk_key.ensure((size_t)n_dir);
    if (e == hipSuccess) e = c->topk_val.ensure((size_t)n_dir);
    const auto packed = rocprim::make_transform_iterator(c->topk_cnt.p, TopkPack{(uint32_t)K});
    size_t tmp_bytes = 0;
    if (e == hipSuccess) e = rocprim::exclusive_scan(nullptr, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream);
    if (e == hipSuccess) e = c->topk_tmp.ensure(tmp_bytes + 256);
    if (e != hipSuccess) {
        set_err(&c->err, "%s top-k: scratch for %llu selected pairs of %lld %s: %s", pass, n, (long long)n_own, job.owner_pl, hipGetErrorString(e));
        return SELHIP_E_HIP;
    }
    u64 totals = 0;
    bool have_totals = false;
    const auto read_totals = [&]() -> int {
        HIPCHK(&c->err, hipMemcpyAsync(&totals, c->topk_off.p + n_own, sizeof(u64), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(&c->err, hipStreamSynchronize(c->stream));
        if ((uint32_t)totals != (uint32_t)n_dir) {
            set_err(&c->err, "%s top-k: %u of %llu %srecords carry a %s rank (internal error)", pass, (uint32_t)totals, n_dir,
                    job.both ? "directed " : "", job.owner);
            return SELHIP_E_HIP;
        }
        have_totals = true;
        return SELHIP_OK;
    };
    {
        TimerScope t(c, T_TOPK);
        const unsigned blocks = grid_for(n, kWavesPerBlock * kTopkTile * kWave, 4096);
        const auto count = job.both ? topk_count_kernel<true> : topk_count_kernel<false>;
        const auto scatter = job.both ? topk_scatter_kernel<true> : topk_scatter_kernel<false>;
        HIPCHK(&c->err, hipMemsetAsync(c->topk_cnt.p, 0, 2 * slots * sizeof(uint32_t), c->stream));
        const unsigned blocks_c = grid_for(job.n_carry, kWavesPerBlock * kTopkTile * kWave, 4096);
        if (job.n_carry) {
            hipLaunchKernelGGL(topk_count_kernel<false>, dim3(blocks_c), dim3(kBlock), 0, c->stream, out.p, job.n_carry, (int)n_own, c->topk_cnt.p);
            HIPCHK(&c->err, hipGetLastError());
        }
        hipLaunchKernelGGL(count, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_own, c->topk_cnt.p);
        HIPCHK(&c->err, hipGetLastError());
        tmp_bytes = c->topk_tmp.cap;
        HIPCHK(&c->err, rocprim::exclusive_scan(c->topk_tmp.p, tmp_bytes, packed, c->topk_off.p, (u64)0, slots, rocprim::plus<u64>(), c->stream));
        if (job.n_carry) {
            hipLaunchKernelGGL(topk_scatter_kernel<false>, dim3(blocks_c), dim3(kBlock), 0, c->stream, out.p, job.n_carry, (int)n_own, c->topk_off.p,
                               c->topk_cnt.p + slots, c->topk_key.p, c->topk_val.p, n_dir);
            HIPCHK(&c->err, hipGetLastError());
        }
        hipLaunchKernelGGL(scatter, dim3(blocks), dim3(kBlock), 0, c->stream, c->results.p, n, (int)n_own, c->topk_off.p,
                           c->topk_cnt.p + slots, c->topk_key.p, c->topk_val.p, n_dir);
        HIPCHK(&c->err, hipGetLastError());
        // the reduced list holds sum_o min(L_o, K) <= min(n_dir, owners K) records: only where that bound does not fit is the exact
        // count read before the select, and the result buffer grown to it.  Never behind a query pass: the reduced list is no longer
        // than the list it replaces, and an accepted pass has n_results <= results.cap
        // (a merge: C is dead behind its scatter, like the pass's own records, so the list that replaces it may move)
        if (std::min<u64>(n_dir, (u64)n_own * (u64)K) > (u64)out.cap) {
            const int rc = read_totals();
            if (rc) return rc;
            const size_t need = (size_t)(totals >> 32);
            // (C grows from round to round until every owner holds K: twice what it needs now, so that it moves a few times only)
            if (need > out.cap && (e = out.ensure(job.merge ? std::min<size_t>(2 * need, (size_t)n_own * (size_t)K) : need)) != hipSuccess) {
                set_err(&c->err, "%s top-k: result list of %zu records: %s", pass, need, hipGetErrorString(e));
                return SELHIP_E_HIP;
            }
        }
        hipLaunchKernelGGL(topk_select_kernel, dim3((unsigned)n_own), dim3(kTopkBlock), kTopkLdsBytes, c->stream, c->topk_key.p, c->topk_val.p,
                           c->topk_off.p, K, out.p, (u64)out.cap);
        HIPCHK(&c->err, hipGetLastError());
        if (job.merge) {
            hipLaunchKernelGGL(topk_threshold_kernel, dim3((unsigned)((n_own + kBlock - 1) / kBlock)), dim3(kBlock), 0, c->stream, out.p, (u64)out.cap,
                               c->topk_off.p, (int)n_own, K, c->topk_thr.p);
            HIPCHK(&c->err, hipGetLastError());
        }
    }
    if (!have_totals) { const int rc = read_totals(); if (rc) return rc; }
    c->topk_n = (int64_t)(totals >> 32);
    return SELHIP_OK;
}

}  // namespace

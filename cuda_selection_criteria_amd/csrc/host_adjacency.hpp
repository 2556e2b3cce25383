// host_adjacency.hpp -- host side of the sparse adjacency (kernel_adjacency.cuh; include/selection_hip.h section 2n): the scratch, the
// chain of launches behind selhip_ctx_adjacency and selhip_adjacency, and the context call's checks.  The chain waits for the stream
// once, behind the scan of the kept counts (nnz decides between the compaction and SELHIP_E_OVERFLOW), and once behind the compaction.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_forest.hpp); not a stand-alone header.
#pragma once

namespace {

struct AdjWiden { __host__ __device__ u64 operator()(uint32_t c) const { return (u64)c; } };

// what a chain found: nnz, the rows of the block and long classes, what the count kernel refused
struct AdjResult { int64_t nnz = 0, mid_rows = 0, long_rows = 0; ClusterBad bad{0, ~0ull}; };

hipError_t AdjScratch::ensure(size_t n_rows, size_t entries, size_t tmp_bytes, bool twin) {
    const size_t slots = n_rows + 1;
    hipError_t e = words.ensure(3 * slots + 2 + 2 * n_rows);
    if (e == hipSuccess) e = off.ensure(slots);
    if (e == hipSuccess) e = key.ensure(std::max<size_t>(entries, 1));
    if (e == hipSuccess) e = col.ensure(std::max<size_t>(entries, 1));
    if (e == hipSuccess && twin) e = key2.ensure(entries);
    if (e == hipSuccess && twin) e = col2.ensure(entries);
    if (e == hipSuccess) e = tmp.ensure(tmp_bytes + 256);
    if (e == hipSuccess) e = bad.ensure(2);
    return e;
}

// The chain over n_rec > 0 records and n_rows > 0 rows on st.  SELHIP_OK with res->bad.count != 0: the list holds a rank out of range,
// the outputs are unspecified and the caller reports it.  SELHIP_E_OVERFLOW: d_row_ptr and res->nnz are complete
template <class List>
int adj_run(std::string* err, hipStream_t st, AdjScratch& s, const List& list, u64 n_rec, int64_t n_rows, int64_t n_cols, int form, double min_value,
            const selhip_csr_t& out, int64_t cap, AdjResult* res) {
    const bool sym = form == SELHIP_ADJ_SYMMETRIC;
    const u64 entries = sym ? 2 * n_rec : n_rec;            // the most there can be
    const size_t slots = (size_t)n_rows + 1;
    const bool twin = entries > (u64)kAdjLdsCap;            // (no row can be long otherwise)
    size_t tmp_a = 0, tmp_b = 0;
    hipError_t e = rocprim::exclusive_scan(nullptr, tmp_a, rocprim::make_transform_iterator((uint32_t*)nullptr, AdjWiden{}), (u64*)nullptr, (u64)0, slots,
                                           rocprim::plus<u64>(), st);
    tmp_b = tmp_a;                                          // (the second scan has the first's types and size)
    if (e == hipSuccess) e = s.ensure((size_t)n_rows, (size_t)entries, std::max(tmp_a, tmp_b), twin);
    if (e != hipSuccess) {
        set_err(err, "adjacency: scratch for %llu entries in %lld rows: %s", entries, (long long)n_rows, hipGetErrorString(e));
        return e == hipErrorOutOfMemory ? SELHIP_E_NOMEM : SELHIP_E_HIP;
    }
    uint32_t* const cnt = s.words.p, * const cur = cnt + slots, * const kept = cur + slots, * const ctl = kept + slots;
    uint32_t* const mid_list = ctl + 2, * const long_list = mid_list + n_rows;
    const size_t n_clear = 3 * slots + 2;
    hipLaunchKernelGGL(adj_init_kernel, dim3(grid_for(n_clear, kBlock, 1024)), dim3(kBlock), 0, st, s.words.p, (u64)n_clear, s.bad.p);
    const unsigned blocks = grid_for(n_rec, kWavesPerBlock * kTopkTile * kWave, 4096);
    const auto count = sym ? adj_count_kernel<List, true> : adj_count_kernel<List, false>;
    const auto scatter = sym ? adj_scatter_kernel<List, true> : adj_scatter_kernel<List, false>;
    hipLaunchKernelGGL(count, dim3(blocks), dim3(kBlock), 0, st, list, n_rec, (int)n_rows, (int)n_cols, min_value, cnt, s.bad.p);
    HIPCHK(err, hipGetLastError());
    size_t tmp_bytes = s.tmp.cap;
    HIPCHK(err, rocprim::exclusive_scan(s.tmp.p, tmp_bytes, rocprim::make_transform_iterator(cnt, AdjWiden{}), s.off.p, (u64)0, slots, rocprim::plus<u64>(), st));
    hipLaunchKernelGGL(scatter, dim3(blocks), dim3(kBlock), 0, st, list, n_rec, (int)n_rows, (int)n_cols, min_value, (const u64*)s.off.p, cur, s.key.p,
                       s.col.p, entries, s.bad.p + 1);
    hipLaunchKernelGGL(adj_sort_wave_kernel, dim3(grid_for((u64)n_rows, kWavesPerBlock, 8192)), dim3(kBlock), 0, st, (const u64*)s.off.p, (int)n_rows, s.key.p,
                       s.col.p, kept, ctl, mid_list, long_list);
    HIPCHK(err, hipGetLastError());
    const unsigned list_blocks = (unsigned)std::min<int64_t>(n_rows, kAdjListBlocks);
    if (entries > (u64)kWave)
        hipLaunchKernelGGL(adj_sort_block_kernel, dim3(list_blocks), dim3(kAdjBlock), kAdjLdsBytes, st, (const u64*)s.off.p, s.key.p, s.col.p, kept,
                           (const uint32_t*)ctl, (const uint32_t*)mid_list, (int)n_rows);
    if (twin)
        hipLaunchKernelGGL(adj_sort_long_kernel, dim3(list_blocks), dim3(kAdjBlock), kAdjLdsBytes, st, (const u64*)s.off.p, (int)n_cols, s.key.p, s.col.p,
                           s.key2.p, s.col2.p, kept, (const uint32_t*)ctl, (const uint32_t*)long_list, (int)n_rows);
    HIPCHK(err, hipGetLastError());
    tmp_bytes = s.tmp.cap;
    HIPCHK(err, rocprim::exclusive_scan(s.tmp.p, tmp_bytes, rocprim::make_transform_iterator(kept, AdjWiden{}), reinterpret_cast<u64*>(out.d_row_ptr), (u64)0,
                                        slots, rocprim::plus<u64>(), st));
    uint32_t h_ctl[2] = {0, 0};
    int64_t nnz = 0;
    HIPCHK(err, hipMemcpyAsync(&nnz, out.d_row_ptr + n_rows, sizeof nnz, hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipMemcpyAsync(h_ctl, ctl, sizeof h_ctl, hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipMemcpyAsync(&res->bad, s.bad.p, sizeof(ClusterBad), hipMemcpyDeviceToHost, st));
    HIPCHK(err, hipStreamSynchronize(st));
    res->nnz = nnz; res->mid_rows = h_ctl[0]; res->long_rows = h_ctl[1];
    if (res->bad.count) return SELHIP_OK;
    if (nnz < 0 || (u64)nnz > entries) { set_err(err, "adjacency: %lld entries kept of at most %llu (internal error)", (long long)nnz, entries); return SELHIP_E_HIP; }
    if (nnz > cap) {
        set_err(err, "adjacency: %lld entries, room for %lld (d_row_ptr is complete; at most %llu for this list)", (long long)nnz, (long long)cap, entries);
        return SELHIP_E_OVERFLOW;
    }
    if (nnz > 0) {
        hipLaunchKernelGGL(adj_compact_kernel, dim3(grid_for((u64)nnz, kBlock, 8192)), dim3(kBlock), 0, st, (const int64_t*)out.d_row_ptr, (int)n_rows,
                           (const u64*)s.off.p, (const u64*)s.key.p, (const uint32_t*)s.col.p, entries, nnz, out.d_col, out.d_val);
        HIPCHK(err, hipGetLastError());
        HIPCHK(err, hipStreamSynchronize(st));
    }
    return SELHIP_OK;
}

// what both entries ask of their arguments; who: the entry's name
int adj_check_args(std::string* err, const char* who, int form, double min_value, const selhip_csr_t* out, int64_t cap) {
    if (!out || !out->d_row_ptr) { set_err(err, "%s: null selhip_csr_t or d_row_ptr (d_val may be null, and d_col where cap is 0)", who); return SELHIP_E_BADARG; }
    if (form != SELHIP_ADJ_DIRECTED && form != SELHIP_ADJ_SYMMETRIC) { set_err(err, "%s: form %d (SELHIP_ADJ_DIRECTED or SELHIP_ADJ_SYMMETRIC)", who, form); return SELHIP_E_BADARG; }
    if (std::isnan(min_value)) { set_err(err, "%s: min_value is NaN (-INFINITY takes every record)", who); return SELHIP_E_BADARG; }
    if (cap < 0 || (cap > 0 && !out->d_col)) { set_err(err, "%s: cap >= 0, and d_col wherever cap > 0", who); return SELHIP_E_BADARG; }
    if ((reinterpret_cast<uintptr_t>(out->d_row_ptr) & 7) || (reinterpret_cast<uintptr_t>(out->d_col) & 3) || (reinterpret_cast<uintptr_t>(out->d_val) & 7)) {
        set_err(err, "%s: d_row_ptr and d_val 8-byte aligned, d_col 4-byte aligned", who);
        return SELHIP_E_BADARG;
    }
    return SELHIP_OK;
}

// a list with no entry: d_row_ptr = n_rows + 1 zeros, on st, waited for
int adj_empty(std::string* err, hipStream_t st, int64_t n_rows, const selhip_csr_t& out) {
    hipLaunchKernelGGL(adj_init_kernel, dim3(grid_for(2 * (u64)(n_rows + 1), kBlock, 1024)), dim3(kBlock), 0, st, reinterpret_cast<uint32_t*>(out.d_row_ptr),
                       2 * (u64)(n_rows + 1), (ClusterBad*)nullptr);
    HIPCHK(err, hipGetLastError());
    HIPCHK(err, hipStreamSynchronize(st));
    return SELHIP_OK;
}

int adjacency_call(selhip_ctx* c, int form, double min_value, const selhip_csr_t* out, int64_t cap, int64_t* nnz_out) {
    const char* const who = "selhip_ctx_adjacency";
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", who); return SELHIP_E_STATE; }
    if (!c->have_run) { set_err(&c->err, "%s: the context holds no result list (run a pass first)", who); return SELHIP_E_STATE; }
    if (const int rc = adj_check_args(&c->err, who, form, min_value, out, cap)) return rc;
    if (c->last_was_query && form == SELHIP_ADJ_SYMMETRIC) {
        set_err(&c->err, "%s: the result list is a query pass's, whose ranks live in two index spaces; take SELHIP_ADJ_DIRECTED (n_q rows, n_d columns)", who);
        return SELHIP_E_STATE;
    }
    const int64_t n_rows = c->last_was_query ? c->q.n : c->n, n_cols = c->n, cnt = result_records(c);
    if (n_rows < 0) { set_err(&c->err, "%s: the queries of the last pass are gone", who); return SELHIP_E_STATE; }
    if (n_rows > 0x7FFFFFFFll || n_cols > 0x7FFFFFFFll || cnt > 0x7FFFFFFFll) {
        set_err(&c->err, "%s takes up to 2^31 - 1 rows, columns and records", who);
        return SELHIP_E_BADARG;
    }
    HIPCHK(&c->err, hipSetDevice(c->device));
    AdjResult res;
    int rc;
    {
        TimedCall call(c, T_ADJACENCY);
        TimerScope t(c, T_ADJACENCY);
        rc = n_rows == 0 || cnt == 0 ? adj_empty(&c->err, c->stream, n_rows, *out)
                                     : adj_run(&c->err, c->stream, c->adj, AdjRecordList{c->results.p}, (u64)cnt, n_rows, n_cols, form, min_value, *out, cap, &res);
    }
    if (rc && rc != SELHIP_E_OVERFLOW) return rc;
    if (res.bad.count) {
        set_err(&c->err, "%s: %llu records of the result list carry a rank outside [0, %lld) x [0, %lld); record %llu is one (internal error)", who, res.bad.count,
                (long long)n_rows, (long long)n_cols, res.bad.index);
        return SELHIP_E_HIP;
    }
    c->adjacency_nnz_last = (int)std::min<int64_t>(res.nnz, 0x7FFFFFFF);
    c->adjacency_long_rows_last = (int)res.long_rows;
    c->adjacency_mid_rows_last = (int)res.mid_rows;
    if (nnz_out) *nnz_out = res.nnz;
    return rc;
}

}  // namespace

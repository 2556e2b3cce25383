// abi_merge.inc -- the C ABI of the merge by group (include/selection_hip.h sections 2i and 3): selhip_ctx_merge_groups over the set a
// context holds, selhip_merge_sketches over a caller's rows.  Kernels in kernel_merge.cuh, host side in host_merge.hpp; touches none of
// the passes' state (result list, counters, statistics, top-k, signature cache, "clusters_last").
// Included by selection_kernels.hip.

extern "C" {

int selhip_ctx_merge_groups(selhip_ctx* c, const int32_t* d_group, int64_t n_groups, const selhip_merged_t* out) {
    return merge_groups_call(c, d_group, n_groups, out);
}

int selhip_merge_sketches(const uint8_t* d_hll, const uint64_t* d_smh, const uint8_t* d_aux_hll, int64_t n, int p, int m, int p_aux,
                          const int32_t* d_group, int64_t n_groups, uint8_t* d_hll_out, uint64_t* d_smh_out, uint8_t* d_aux_out,
                          int32_t* d_size_out, void* hip_stream) {
    return merge_sketches_call(d_hll, d_smh, d_aux_hll, n, p, m, p_aux, d_group, n_groups, d_hll_out, d_smh_out, d_aux_out, d_size_out,
                               (hipStream_t)hip_stream);
}

}  // extern "C"

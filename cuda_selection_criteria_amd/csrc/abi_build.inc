// abi_build.inc -- the C ABI of the split sketch builder (include/selection_hip.h section 4b): selhip_build_sketches_split and its plan,
// selhip_build_split_plan.  Kernels in kernel_sketch.cuh, the plan in host_plan.hpp, the host side in host_build.hpp;
// selhip_build_sketches itself is in abi_blocks.inc.
// Included by selection_kernels.hip.

extern "C" {

int selhip_build_sketches_split(const uint8_t* d_codes, const int64_t* d_offsets, const int64_t* h_offsets, int64_t n_genomes, int k, int m, int p_aux,
                                int64_t chunk, uint8_t* d_hll, uint64_t* d_smh, uint8_t* d_aux_hll, selhip_build_info_t* info, void* hip_stream) {
    return build_sketches_split_call(d_codes, d_offsets, h_offsets, n_genomes, k, m, p_aux, chunk, d_hll, d_smh, d_aux_hll, info, (hipStream_t)hip_stream);
}

int selhip_build_split_plan(const int64_t* h_offsets, int64_t n_genomes, int k, int m, int p_aux, int64_t chunk, int64_t resident_blocks,
                            int64_t* chunk_counts, selhip_build_info_t* info) {
    if (!info) { set_err(nullptr, "selhip_build_split_plan: null selhip_build_info_t"); return SELHIP_E_BADARG; }
    return build_split_plan_call(h_offsets, n_genomes, k, m, p_aux, chunk, resident_blocks, chunk_counts, info, nullptr, "selhip_build_split_plan");
}

}  // extern "C"

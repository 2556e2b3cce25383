// abi_gather.inc -- the C ABI of the winner-takes-all screen (include/selection_hip.h sections 2m and 3): selhip_ctx_gather over a
// context's attached queries and database, selhip_gather over a caller's bucket rows.  Kernels in kernel_gather.cuh, host side in
// host_gather.hpp; touches none of the passes' state and none of the other calls' timers.
// Included by selection_kernels.hip, behind abi_nj.inc.

extern "C" {

int selhip_ctx_gather(selhip_ctx* c, int c_min, int max_picks, selhip_gather_pick_t* d_picks, int32_t* d_n_picks, int32_t* d_unexplained) {
    return gather_ctx_call(c, c_min, max_picks, d_picks, d_n_picks, d_unexplained);
}

int selhip_gather(const uint64_t* d_q_aux, int64_t n_q, const uint64_t* d_db_aux, int64_t n_d, int m, int c_min, int max_picks,
                  selhip_gather_pick_t* d_picks, int32_t* d_n_picks, int32_t* d_unexplained, void* hip_stream) {
    const char* const what = "selhip_gather";
    if (const int rc = gather_check(nullptr, what, m, c_min, max_picks, d_picks, d_n_picks, d_unexplained)) return rc;
    if (n_q < 0 || n_q > 0x7FFFFFFFll || n_d < 0 || n_d > 0x7FFFFFFFll || (n_q > 0 && !d_q_aux) || (n_q > 0 && n_d > 0 && !d_db_aux) ||
        (reinterpret_cast<uintptr_t>(d_q_aux) & 7) || (reinterpret_cast<uintptr_t>(d_db_aux) & 7)) {
        set_err(nullptr, "%s: 0 <= n_q, n_d <= 2^31 - 1, non-null 8-byte aligned bucket rows where there is something to read", what);
        return SELHIP_E_BADARG;
    }
    if (n_q == 0) return SELHIP_OK;
    int cap = 0, kind = 0;
    if (gather_device_lds(&cap)) { set_err(nullptr, "%s: the device reports no LDS size", what); return SELHIP_E_HIP; }
    return gather_run(nullptr, nullptr, what, (hipStream_t)hip_stream, reinterpret_cast<const u64*>(d_q_aux), n_q, reinterpret_cast<const u64*>(d_db_aux), n_d, m,
                      c_min, max_picks, cap, GatherOut{d_picks, d_n_picks, d_unexplained}, false, &kind);
}

}  // extern "C"

// host_graph.hpp -- the front end the three graph calls share on the host (single-linkage clusters, greedy representative clusters,
// maximum spanning forest; host_cluster.hpp, host_greedy.hpp, host_forest.hpp keep their own launches and rounds).  For the context
// calls over the result list: the admission checks and the run of an admitted call (its timer, the split into no genome / no record /
// the launches, the report of records with a rank out of range); their scratch is GraphScratch, in host_context.hpp.  For the
// free-standing entries over a caller's list: the empty vertex set, the report of invalid entries, and DevBlock, the one allocation
// of a call carved into its arrays.
// Part of the kernel translation unit selection_kernels.hip (included there, after host_topk.hpp); not a stand-alone header.
#pragma once

namespace {

// how a context call names itself in its messages, and its timer
struct GraphCall { const char* entry; const char* out_struct; const char* advice; int timer; };
constexpr GraphCall kClusterCall{"selhip_ctx_cluster", "selhip_clusters_t", "cluster", T_CLUSTER};
constexpr GraphCall kGreedyCall{"selhip_ctx_cluster_greedy", "selhip_greedy_t", "cluster", T_GREEDY};
constexpr GraphCall kForestCall{"selhip_ctx_spanning_forest", "selhip_forest_t", "take", T_FOREST};

// the checks every context call makes, in the order it makes them; own_checks() -- the call's own arguments (rep_rule / order_rule,
// d_priority), SELHIP_OK or an error it has reported -- runs in front of the size limit, where those checks have always run
template <class Own>
int graph_admit(selhip_ctx* c, const GraphCall& d, const void* out, double min_value, Own&& own_checks) {
    if (!c) return SELHIP_E_BADARG;
    if (c->pending) { set_err(&c->err, "%s: a pass is still pending (selhip_ctx_finish)", d.entry); return SELHIP_E_STATE; }
    if (!c->have_run) { set_err(&c->err, "%s: the context holds no result list (run a pass first)", d.entry); return SELHIP_E_STATE; }
    if (c->last_was_query) {
        set_err(&c->err, "%s: the result list is a query pass's, whose ranks live in two index spaces; %s an all-pairs or pair-list pass", d.entry, d.advice);
        return SELHIP_E_STATE;
    }
    if (!out) { set_err(&c->err, "%s: null %s (its members may be null, the struct may not)", d.entry, d.out_struct); return SELHIP_E_BADARG; }
    if (std::isnan(min_value)) { set_err(&c->err, "%s: min_value is NaN (-INFINITY takes every record)", d.entry); return SELHIP_E_BADARG; }
    if (const int rc = own_checks()) return rc;
    if (c->n > 0x7FFFFFFFll) { set_err(&c->err, "%s takes up to 2^31 - 1 genomes", d.entry); return SELHIP_E_BADARG; }
    return SELHIP_OK;
}

// an admitted call, timed under d.timer per call.  No genome: nothing to write.  No record, no edge: singletons() enqueues the one
// launch that writes the whole answer, and is waited for.  Else launches(cnt, &bad) -- n > 0 vertices, cnt > 0 records -- which
// returns with the stream idle and what its edge kernel refused in bad
template <class Singletons, class Launches>
int graph_run(selhip_ctx* c, const GraphCall& d, Singletons&& singletons, Launches&& launches) {
    const int64_t n = c->n, cnt = result_records(c);
    HIPCHK(&c->err, hipSetDevice(c->device));
    int rc = SELHIP_OK;
    ClusterBad bad{0, ~0ull};
    {
        TimedCall call(c, d.timer);
        if (n > 0 && cnt == 0) {
            {
                TimerScope t(c, d.timer);
                singletons();
            }
            hipError_t e = hipGetLastError();
            if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
            if (e != hipSuccess) { set_err(&c->err, "%s: %s", d.entry, hipGetErrorString(e)); rc = SELHIP_E_HIP; }
        } else if (n > 0) {
            rc = launches(cnt, &bad);
        }
    }
    if (rc) return rc;
    if (bad.count) {
        set_err(&c->err, "%s: %llu records of the result list carry a rank outside [0, %lld); record %llu is one (internal error)", d.entry, bad.count,
                (long long)n, bad.index);
        return SELHIP_E_HIP;
    }
    return SELHIP_OK;
}

// a free-standing entry without vertices: nothing to do, unless its list has entries -- every one of them invalid
int graph_no_vertices(int64_t n_pairs) {
    if (n_pairs == 0) return SELHIP_OK;
    set_err(nullptr, "the pair list holds %lld invalid entries (a vertex outside [0, 0)); entry 0 is one", (long long)n_pairs);
    return SELHIP_E_BADARG;
}
// ... and what its edge kernel refused, over n vertices
int graph_bad_entries(const ClusterBad& bad, int64_t n) {
    if (!bad.count) return SELHIP_OK;
    set_err(nullptr, "the pair list holds %llu invalid entries (a vertex outside [0, %lld)); entry %llu is one", bad.count, (long long)n, bad.index);
    return SELHIP_E_BADARG;
}

// one hipMalloc carved into arrays of the types T..., count[i] elements of the i-th, each starting on a 16-byte boundary; freed with
// the object.  The total and the pointers come from the one list, so they cannot disagree
template <class... T>
struct DevBlock {
    char* base = nullptr;
    size_t off[sizeof...(T) + 1] = {};                                        // where part i starts; the last: the total
    hipError_t alloc(const size_t (&count)[sizeof...(T)]) {
        const size_t size[] = {sizeof(T)...};
        for (size_t i = 0; i < sizeof...(T); ++i) off[i + 1] = off[i] + ((count[i] * size[i] + 15) & ~(size_t)15);
        return hipMalloc((void**)&base, off[sizeof...(T)]);
    }
    template <size_t I>
    auto part() const { return reinterpret_cast<std::tuple_element_t<I, std::tuple<T...>>*>(base + off[I]); }
    DevBlock() = default;
    DevBlock(const DevBlock&) = delete;
    ~DevBlock() { if (base) (void)hipFree(base); }
};

}  // namespace

// kernel_greedy.cuh -- greedy representative clusters of a record list (selhip_greedy_representatives, selhip_ctx_cluster_greedy; host
// side in host_greedy.hpp): the CD-HIT / UCLUST scheme.  Part of libselhip.so; included by selection_kernels.hip only, behind
// kernel_graph.cuh (the lists, graph_edge, graph_image, cl_degree_add) and kernel_cluster.cuh, whose cluster_rep_key it reuses.
//
// THE SEQUENTIAL DEFINITION.  Every vertex has a 64-bit key; a vertex h goes BEFORE a vertex l when key[h] > key[l], or the keys are
// equal and h < l (greedy_before).  Visit the vertices in that order: a vertex becomes a representative unless one of its neighbours
// already is one.  The representatives are the lexicographically first maximal independent set of the graph under the order.
//
// THE ROUNDS.  state[n] holds UNDECIDED, REP or MEMBER; blocked[n] the last round in which a vertex was held back.  Round r = 1, 2, ...:
//   greedy_edges_kernel    one lane per record, grid-stride.  For an edge with the earlier end h and the later end l, l still UNDECIDED:
//                            state[h] == REP        state[l] = MEMBER
//                            state[h] == UNDECIDED  blocked[l] = r
//                            state[h] == MEMBER     nothing
//   greedy_vertices_kernel a vertex that is UNDECIDED and has blocked[g] != r becomes REP; those that stay UNDECIDED are counted
// until the count is zero.  The host reads the count after a batch of rounds; a round that starts with a count of zero returns at once.
//
// WHY ANY INTERLEAVING GIVES THE SEQUENTIAL ANSWER.  A vertex turns REP only when every neighbour before it is MEMBER (none of them REP,
// which would have made it MEMBER; none UNDECIDED, which would have blocked it), and it turns MEMBER only behind a REP neighbour that
// goes before it.  Both states are final.  By induction over the order the decided vertices therefore carry exactly the sequential
// greedy's decisions: the first vertex of the order has nothing before it and is REP after round 1; a vertex whose earlier neighbours
// are all decided correctly is MEMBER if and only if one of them is REP, as the sequential visit decides.  Inside greedy_edges_kernel
// state[] is read with plain loads while other lanes store MEMBER into it, so a read can be STALE: UNDECIDED for a vertex another
// lane has just made MEMBER, or a MEMBER store of this launch not yet visible across CUs or XCDs (the vector L1 is per CU, the L2s of
// the eight XCDs are not coherent with each other).  REP is never stored in that kernel, so the only stale value is UNDECIDED for a
// MEMBER, and acting on it only blocks l for one more round (h stale) or stores MEMBER / blocked onto a vertex that is MEMBER already
// (l stale; greedy_vertices_kernel looks at blocked[] only for an UNDECIDED vertex): a stale read can delay a decision, never change
// it.  Every store into state[] or blocked[] from several lanes stores the same value (MEMBER, or the round).  The first UNDECIDED
// vertex of the order is decided in every round -- everything before it is decided, so it is MEMBER behind a REP or unblocked -- so
// at most n rounds are needed; with all reads stale the count is that of the synchronous scheme, the upper bound of any run.
//
// No loop waits for the progress of another lane, wave or block: no spin, no flag poll, no grid barrier, no cooperative launch, no
// inline assembly.  Visibility BETWEEN the rounds comes from the kernel boundary alone.  The outputs behind the rounds are integer
// atomic maxima, minima and adds without a return value: order-independent, so every output is bit-reproducible.
//   greedy_key_kernel      key[g] by the order rule, built ONCE per call (two 8-byte gathers per live edge and round, instead of the
//                          degrees and the rule's arithmetic in every round)
//   greedy_degree_kernel   the degree tally of cluster_edges_kernel alone (cl_degree_add), launched only where a degree is wanted
//   greedy_reps_kernel     rep_of[g] = g or none yet, the representatives' flags for the scan
//   greedy_best_kernel     per member, the greatest value of an edge to a representative: a 64-bit atomic maximum on graph_image(value)
//   greedy_assign_kernel   the records whose value is the member's best and whose other end is REP: an atomic minimum on its rank
//                          (two passes: value and rank do not fit one 64-bit atomic)
//   (rocprim::exclusive_scan of the flags: the dense ids, numbered by ascending representative)
//   greedy_members_kernel  value[g], members per representative;  greedy_write_kernel  cluster[g], cluster_size[c], cluster_rep[c]
//   greedy_singletons_kernel  the whole answer of a list without records, in the one launch
#pragma once

namespace {

enum : int { kGreedyUndecided = 0, kGreedyRep = 1, kGreedyMember = 2 };
constexpr int kGreedyNone = 0x7FFFFFFF;        // rep_of of a member before greedy_assign_kernel: above every rank

// h goes before l in the visiting order
__device__ __forceinline__ bool greedy_before(u64 key_h, int h, u64 key_l, int l) { return key_h > key_l || (key_h == key_l && h < l); }

// key[g]: SELHIP_REP_MAX_DEGREE, _MIN_RANK, _MAX_RANK as cluster_rep_key; SELHIP_REP_PRIORITY (priority[g], reversed rank); the state
// and the tallies of a call cleared.  Every pointer but state / blocked / key may be null
__global__ void __launch_bounds__(kBlock)
greedy_key_kernel(long long n, int rule, const int* __restrict__ degree, const uint32_t* __restrict__ priority, const u64* __restrict__ caller_key,
                  u64* __restrict__ key, int* __restrict__ state, int* __restrict__ blocked, u64* __restrict__ best, int* __restrict__ members) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        key[g] = caller_key ? caller_key[g]
               : rule == SELHIP_REP_PRIORITY ? ((u64)priority[g] << 32) | (0xFFFFFFFFull - (u64)(uint32_t)g)
               : cluster_rep_key(rule, (int)g, degree ? degree[g] : 0);
        state[g] = kGreedyUndecided;
        blocked[g] = 0;
        if (best) best[g] = 0;
        if (members) members[g] = 0;
    }
}

// degree[] = 0 and the tally of what a list holds that is no vertex
__global__ void __launch_bounds__(kBlock)
greedy_clear_kernel(long long n, int* __restrict__ degree, ClusterBad* __restrict__ bad) {
    const long long stride = (long long)gridDim.x * kBlock;
    if (degree) for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) degree[g] = 0;
    if (blockIdx.x == 0 && threadIdx.x == 0) { bad->count = 0; bad->index = ~0ull; }
}

// every record of the graph adds one to both of its vertices, a record with i == k two to the one: the tally of cluster_edges_kernel
template <class List>
__global__ void __launch_bounds__(kBlock)
greedy_degree_kernel(const List list, u64 n_edges, int n, int* __restrict__ degree) {
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        double value;
        const bool ok = graph_edge<true>(list, e, n, &u, &v, &value, nullptr);
        cl_degree_add(degree, u, ok);
        cl_degree_add(degree, v, ok);
    }
}

// one round's pass over the records (see the head of the file).  prev (may be null): the UNDECIDED count behind the round before; zero
// means the selection is complete and this launch has nothing to do.  bad: non-null in round 1 alone
template <class List>
__global__ void __launch_bounds__(kBlock)
greedy_edges_kernel(const List list, u64 n_edges, int n, const u64* __restrict__ key, int* state, int* blocked, int round,
                    const uint32_t* __restrict__ prev, ClusterBad* __restrict__ bad) {
    if (prev && *prev == 0) return;
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        double value;
        if (!graph_edge<true>(list, e, n, &u, &v, &value, bad) || u == v) continue;
        const int su = state[u], sv = state[v];
        if (su != kGreedyUndecided && sv != kGreedyUndecided) continue;             // both ends final: most records, after a few rounds
        const bool u_first = greedy_before(key[u], u, key[v], v);
        const int l = u_first ? v : u, sh = u_first ? su : sv, sl = u_first ? sv : su;
        if (sl != kGreedyUndecided) continue;
        if (sh == kGreedyRep) state[l] = kGreedyMember;
        else if (sh == kGreedyUndecided) blocked[l] = round;
    }
}

// behind a round's edge kernel: the vertices nothing held back become REP; *undecided (cleared by the host before the batch) counts
// those still UNDECIDED, one add per wave
__global__ void __launch_bounds__(kBlock)
greedy_vertices_kernel(long long n, int* __restrict__ state, const int* __restrict__ blocked, int round, const uint32_t* __restrict__ prev,
                       uint32_t* __restrict__ undecided) {
    if (prev && *prev == 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        bool waits = false;
        if (state[g] == kGreedyUndecided) {
            if (blocked[g] == round) waits = true;
            else state[g] = kGreedyRep;
        }
        const u64 m = __ballot(waits);
        if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(undecided, (uint32_t)__popcll(m));
    }
}

// the selection is complete: is_rep / rep_of / flag (each may be null).  flag[n] = 0: the scan's total lands there
__global__ void __launch_bounds__(kBlock)
greedy_reps_kernel(long long n, const int* __restrict__ state, uint8_t* __restrict__ is_rep, int* __restrict__ rep_of, uint32_t* __restrict__ flag) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        const bool rep = state[g] == kGreedyRep;
        if (is_rep) is_rep[g] = rep ? 1 : 0;
        if (rep_of) rep_of[g] = rep ? (int)g : kGreedyNone;
        if (flag) flag[g] = rep ? 1u : 0u;
    }
    if (flag && blockIdx.x == 0 && threadIdx.x == 0) flag[n] = 0;
}

// best[g] = the greatest image of an edge between the member g and a representative
template <class List>
__global__ void __launch_bounds__(kBlock)
greedy_best_kernel(const List list, u64 n_edges, int n, const int* __restrict__ state, u64* __restrict__ best) {
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        double value;
        if (!graph_edge<true>(list, e, n, &u, &v, &value, nullptr) || u == v) continue;
        const int su = state[u], sv = state[v];
        if (su == sv) continue;                                                      // (two representatives share no edge)
        const int g = su == kGreedyMember ? u : v;
        atomicMax(best + g, graph_image(value));
    }
}

// rep_of[g] = the smallest representative among those the member g has an edge of its best value to
template <class List>
__global__ void __launch_bounds__(kBlock)
greedy_assign_kernel(const List list, u64 n_edges, int n, const int* __restrict__ state, const u64* __restrict__ best, int* __restrict__ rep_of) {
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        double value;
        if (!graph_edge<true>(list, e, n, &u, &v, &value, nullptr) || u == v) continue;
        const int su = state[u], sv = state[v];
        if (su == sv) continue;
        const int g = su == kGreedyMember ? u : v, r = su == kGreedyMember ? v : u;
        if (best[g] == graph_image(value)) atomicMin(rep_of + g, r);
    }
}

// value[g]: 1.0 for a representative, else the member's best value (its record's bits; a zero of either sign is written +0.0);
// members[r] += 1 for every vertex of r's cluster.  value / members may be null
__global__ void __launch_bounds__(kBlock)
greedy_members_kernel(long long n, const int* __restrict__ state, const u64* __restrict__ best, const int* __restrict__ rep_of,
                      double* __restrict__ value, int* __restrict__ members) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        if (value) value[g] = state[g] == kGreedyRep ? 1.0 : graph_value(best[g]);
        if (members) {
            const int r = rep_of[g];
            if ((uint32_t)r < (uint32_t)n) atomicAdd(members + r, 1);
        }
    }
}

// ids[r] = the exclusive scan of the flags: the dense id of the representative r.  cluster / cluster_size / cluster_rep may be null
__global__ void __launch_bounds__(kBlock)
greedy_write_kernel(long long n, const int* __restrict__ state, const int* __restrict__ rep_of, const uint32_t* __restrict__ ids,
                    const int* __restrict__ members, int* __restrict__ cluster, int* __restrict__ cluster_size, int* __restrict__ cluster_rep) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        if (cluster) {
            const int r = rep_of[g];
            cluster[g] = (uint32_t)r < (uint32_t)n ? (int)ids[r] : -1;
        }
        if (state[g] == kGreedyRep) {
            const uint32_t c = ids[g];
            if (cluster_size) cluster_size[c] = members[g];
            if (cluster_rep) cluster_rep[c] = (int)g;
        }
    }
}

// a list without records: every vertex its own representative at value 1.0, with no record.  Every pointer may be null
__global__ void __launch_bounds__(kBlock)
greedy_singletons_kernel(long long n, uint8_t* __restrict__ is_rep, int* __restrict__ rep_of, double* __restrict__ value, int* __restrict__ cluster,
                         int* __restrict__ degree, int* __restrict__ cluster_size, int* __restrict__ cluster_rep) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        if (is_rep) is_rep[g] = 1;
        if (rep_of) rep_of[g] = (int)g;
        if (value) value[g] = 1.0;
        if (cluster) cluster[g] = (int)g;
        if (degree) degree[g] = 0;
        if (cluster_size) cluster_size[g] = 1;
        if (cluster_rep) cluster_rep[g] = (int)g;
    }
}

}  // namespace

// kernel_forest.cuh -- the maximum spanning forest of a record list, which is its single-linkage dendrogram (selhip_spanning_forest,
// selhip_ctx_spanning_forest; host side in host_forest.hpp).  Part of libselhip.so; included by selection_kernels.hip only, behind
// kernel_graph.cuh (cl_load, cl_unite, ClusterBad, graph_image, graph_value, the lists).
//
// THE DEFINITION.  An edge is an unordered pair {a < b} with the greatest value of its records; edge e goes BEFORE edge f when
// image(e) > image(f), or the images are equal and (e.a, e.b) is lexicographically smaller: a strict total order.  Kruskal's visit in
// that order keeps an edge iff its ends are not yet connected; the result is unique.
//
// THE ROUNDS (Boruvka).  comp[n] holds every vertex's component root, best_img[n] / best_pair[n] one 64-bit word per root, parent[n]
// the union-find of kernel_cluster.cuh (parent[x] <= x).  Round r = 1, 2, ...:
//   forest_best_kernel     one lane per record: an edge with comp[a] != comp[b] raises best_img of both components to image(value)
//   forest_pick_kernel     the same stream: where image == best_img[c], best_pair[c] falls to (a << 32) | b  (value and pair do not fit
//                          one 64-bit atomic: two passes, as greedy_best_kernel / greedy_assign_kernel)
//   forest_hook_kernel     one lane per vertex: a root g with a pick finds the other component o, emits {a, b, value} unless o picked the
//                          same edge and o < g (a mutual pick is emitted by the smaller root alone; an edge has two ends, so nothing else
//                          can pick it twice), then cl_unite(parent, g, o)
//   forest_flatten_kernel  comp[g] = root(g), best_* cleared, this round's picks counted
// until a round picks nothing.  The host sorts the emitted records into BEFORE order (rocPRIM merge sort under forest_before).
//
// WHY ANY INTERLEAVING GIVES THE DEFINITION'S FOREST.  A component's pick is its BEFORE-most outgoing edge, which belongs to the unique
// forest by the cut property; under a strict order the picks of a round close no cycle, so cl_unite in any interleaving ends in the same
// partition.  comp[] is written by forest_flatten_kernel alone and read behind a kernel boundary, so every round sees the partition
// of the synchronous scheme and the round count is deterministic: at most ceil(log2 n) rounds that pick, plus the empty one.
//
// HOT WORDS.  Once a giant component exists, millions of records aim at one best_img word.  Two mitigations (forest_aim):
//   * the pre-read: an agent-scope relaxed 8-byte load (cl_load's form; a plain load may sit stale in a CU's L1 for the whole kernel),
//     and no atomic when the lane's value is not beyond what was read.  best_img only rises and best_pair only falls within a launch, so
//     a STALE read is nearer the cleared word than the truth: it can only cause an atomic that changes nothing, never skip one that would.
//     For the same reason a plain load goes in front of it: however stale, what it returns can dismiss a lane and nothing else, and the
//     lanes it dismisses never reach the few hot lines beyond L2 (measured: DESIGN.md section 27);
//   * per-wave aggregation for up to two leaders, as cl_degree_add: the lanes that share the leader's component reduce their value in
//     the wave and the leader issues the one atomic.  Maxima and minima in any grouping give the same word.
// Inside forest_hook_kernel parent[] is shared by every lane: cl_unite's atomics and agent-scope loads, argued in kernel_cluster.cuh.
// best_*, comp[] are read there with plain loads: nothing writes them in that launch.
//
// No loop waits for the progress of another lane, wave or block: no spin, no flag poll, no grid barrier, no cooperative launch, no
// inline assembly.  Visibility BETWEEN the launches comes from the kernel boundary alone.  Every loop over records or vertices is
// bounded by a wave-uniform index, so all 64 lanes reach the cross-lane steps together.  The slots of the emitted records come from an
// atomic add, so their order is arbitrary; the sort behind the rounds makes every output a pure function of the list.
#pragma once

namespace {

constexpr u64 kForestNoPair = ~0ull;            // best_pair of a component without a pick

// a forest edge as the outputs carry it: selhip_pair_t's 16 bytes
struct alignas(16) ForestEdge { int a, b; double value; };
static_assert(sizeof(ForestEdge) == sizeof(selhip_pair_t), "a forest edge is a result record");

// the BEFORE order on emitted records (values are no NaN).  image: graph_image's rule (greedy_image, until the graph kernels shared
// it), written out for the sort's host and device sides -- and for its kernels: through graph_image itself rocPRIM's merge sort
// compiles to other instructions
struct ForestBefore {
    __host__ __device__ static u64 image(double v) {
        if (v == 0.0) v = 0.0;
        u64 b;
        __builtin_memcpy(&b, &v, sizeof b);
        return (b >> 63) ? ~b : b | 0x8000000000000000ull;
    }
    __host__ __device__ bool operator()(const ForestEdge& e, const ForestEdge& f) const {
        const u64 ie = image(e.value), jf = image(f.value);
        if (ie != jf) return ie > jf;
        return e.a != f.a ? e.a < f.a : e.b < f.b;
    }
};

__device__ __forceinline__ u64 fo_load(const u64* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// word[c] = max (kMax) or min of itself and val, for every lane with ok; see HOT WORDS above.  Call with the whole wave converged
template <bool kMax>
__device__ __forceinline__ void forest_aim(u64* __restrict__ word, int c, u64 val, bool ok) {
    if (ok) {
        const u64 near = word[c];                                        // whatever the CU's L1 or the XCD's L2 holds: never beyond the truth
        ok = kMax ? val > near : val < near;
        if (ok) {
            const u64 seen = fo_load(word + c);
            ok = kMax ? val > seen : val < seen;
        }
    }
    const int lane = (int)__lane_id();
    u64 todo = __ballot(ok);
    for (int round = 0; round < 2 && todo; ++round) {                    // (todo is wave-uniform: the loop branches on SGPRs)
        const int leader = __ffsll((long long)todo) - 1;
        const int lc = __builtin_amdgcn_readlane(c, leader);
        const bool mine = ok && c == lc;
        const u64 same = __ballot(mine) & todo;
        u64 m = mine ? val : (kMax ? 0ull : ~0ull);
        if (same & (same - 1)) {                                         // more than one lane: reduce across the wave
            for (int s = 32; s; s >>= 1) {
                const u64 o = __shfl_xor(m, s);
                m = kMax ? (o > m ? o : m) : (o < m ? o : m);
            }
        }
        if (lane == leader) { if (kMax) (void)atomicMax(word + lc, m); else (void)atomicMin(word + lc, m); }
        todo &= ~same;
    }
    if (ok && ((todo >> lane) & 1ull)) { if (kMax) (void)atomicMax(word + c, val); else (void)atomicMin(word + c, val); }
}

// one record as an edge of the graph between two components: a < b, its image, the two roots.  false for a record below the cut, a
// NaN value, a self-loop, an edge inside one component, and a record with a rank outside [0, n), which is tallied in *bad where the
// caller passes it (round 1 does) and indexes nothing
template <class List>
__device__ __forceinline__ bool forest_record(const List& list, u64 e, int n, const int* __restrict__ comp, int* a, int* b, u64* img,
                                              int* ca, int* cb, ClusterBad* __restrict__ bad) {
    int u, v;
    double value;
    if (!list.edge(e, &u, &v, &value)) return false;
    if ((uint32_t)u >= (uint32_t)n || (uint32_t)v >= (uint32_t)n) {                 // (graph_edge's check, written out: folded onto it the
        if (bad) { atomicAdd(&bad->count, 1ull); atomicMin(&bad->index, e); }       // two record kernels compile to other branches)
        return false;
    }
    if (!(value == value) || u == v) return false;
    *a = u < v ? u : v; *b = u < v ? v : u;
    *img = graph_image(value);
    *ca = comp[*a]; *cb = comp[*b];
    return *ca != *cb;
}

// parent[g] = comp[g] = g, the words cleared; the tally of invalid entries, the emitted records and (count may be null) nothing else
__global__ void __launch_bounds__(kBlock)
forest_init_kernel(long long n, int* __restrict__ parent, int* __restrict__ comp, u64* __restrict__ best_img, u64* __restrict__ best_pair,
                   uint32_t* __restrict__ emitted, ClusterBad* __restrict__ bad) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        parent[g] = (int)g; comp[g] = (int)g;
        best_img[g] = 0; best_pair[g] = kForestNoPair;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) { *emitted = 0; bad->count = 0; bad->index = ~0ull; }
}

// prev (may be null): the picks of the round before; zero means the forest is complete and this launch has nothing to do.
// bad: non-null in round 1 alone
template <class List>
__global__ void __launch_bounds__(kBlock)
forest_best_kernel(const List list, u64 n_edges, int n, const int* __restrict__ comp, u64* __restrict__ best_img,
                   const uint32_t* __restrict__ prev, ClusterBad* __restrict__ bad) {
    if (prev && *prev == 0) return;
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 base = (u64)blockIdx.x * kBlock; base < n_edges; base += stride) {      // block-uniform bound: the waves stay whole
        const u64 e = base + threadIdx.x;
        int a = 0, b = 0, ca = 0, cb = 0;
        u64 img = 0;
        const bool ok = e < n_edges && forest_record(list, e, n, comp, &a, &b, &img, &ca, &cb, bad);
        forest_aim<true>(best_img, ca, img, ok);
        forest_aim<true>(best_img, cb, img, ok);
    }
}

template <class List>
__global__ void __launch_bounds__(kBlock)
forest_pick_kernel(const List list, u64 n_edges, int n, const int* __restrict__ comp, const u64* __restrict__ best_img,
                   u64* __restrict__ best_pair, const uint32_t* __restrict__ prev) {
    if (prev && *prev == 0) return;
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 base = (u64)blockIdx.x * kBlock; base < n_edges; base += stride) {
        const u64 e = base + threadIdx.x;
        int a = 0, b = 0, ca = 0, cb = 0;
        u64 img = 0;
        const bool ok = e < n_edges && forest_record(list, e, n, comp, &a, &b, &img, &ca, &cb, nullptr);
        const u64 pair = ((u64)(uint32_t)a << 32) | (u64)(uint32_t)b;
        forest_aim<false>(best_pair, ca, pair, ok && best_img[ca] == img);          // (best_img is final behind the kernel boundary)
        forest_aim<false>(best_pair, cb, pair, ok && best_img[cb] == img);
    }
}

// edges[slot] for slot < cap alone: the forest has at most n - 1 edges, and a store never depends on that being so
__global__ void __launch_bounds__(kBlock)
forest_hook_kernel(long long n, const int* __restrict__ comp, const u64* __restrict__ best_img, const u64* __restrict__ best_pair,
                   int* parent, ForestEdge* __restrict__ edges, uint32_t cap, uint32_t* __restrict__ emitted, const uint32_t* __restrict__ prev) {
    if (prev && *prev == 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    const int lane = (int)__lane_id();
    for (long long base = (long long)blockIdx.x * kBlock; base < n; base += stride) {
        const long long g = base + threadIdx.x;
        u64 pair = kForestNoPair;
        if (g < n && comp[g] == (int)g) pair = best_pair[g];
        const bool picks = pair != kForestNoPair;
        int a = 0, b = 0, o = 0;
        bool emits = false;
        if (picks) {
            a = (int)(uint32_t)(pair >> 32); b = (int)(uint32_t)pair;
            const int ca = comp[a];
            o = ca == (int)g ? comp[b] : ca;
            emits = !(best_pair[o] == pair && o < (int)g);
        }
        const u64 m = __ballot(emits);
        if (m) {                                                                    // one add per wave, the slots by lane order
            const int leader = __ffsll((long long)m) - 1;
            uint32_t first = 0;
            if (lane == leader) first = atomicAdd(emitted, (uint32_t)__popcll(m));
            first = (uint32_t)__builtin_amdgcn_readlane((int)first, leader);
            const uint32_t slot = first + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (emits && slot < cap) {
                const u64 bits = (u64)__double_as_longlong(graph_value(best_img[g]));
                reinterpret_cast<uint4*>(edges)[slot] = make_uint4((uint32_t)a, (uint32_t)b, (uint32_t)bits, (uint32_t)(bits >> 32));
            }
        }
        if (picks) cl_unite(parent, (int)g, o);
    }
}

// behind the hook kernel's end every parent[] value is final and visible: plain loads.  *picks (cleared by the host before the batch)
// counts the roots of this round that had a pick, one add per wave
__global__ void __launch_bounds__(kBlock)
forest_flatten_kernel(long long n, const int* __restrict__ parent, int* __restrict__ comp, u64* __restrict__ best_img, u64* __restrict__ best_pair,
                      const uint32_t* __restrict__ prev, uint32_t* __restrict__ picks) {
    if (prev && *prev == 0) return;
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long base = (long long)blockIdx.x * kBlock; base < n; base += stride) {
        const long long g = base + threadIdx.x;
        bool picked = false;
        if (g < n) {
            int r = (int)g, p = parent[r];
            while (p != r) { r = p; p = parent[r]; }            // r falls strictly: at most g steps
            comp[g] = r;
            picked = best_pair[g] != kForestNoPair;
            best_img[g] = 0; best_pair[g] = kForestNoPair;
        }
        const u64 m = __ballot(picked);
        if (m && (int)__lane_id() == __ffsll((long long)m) - 1) atomicAdd(picks, (uint32_t)__popcll(m));
    }
}

// a list without records: every vertex its own component.  label may be null
__global__ void __launch_bounds__(kBlock)
forest_singletons_kernel(long long n, int* __restrict__ label) {
    const long long stride = (long long)gridDim.x * kBlock;
    if (label) for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) label[g] = (int)g;
}

}  // namespace

// kernel_graph.cuh -- what the three graph calls over a record list share on the device: the single-linkage clusters
// (kernel_cluster.cuh), the greedy representative clusters (kernel_greedy.cuh) and the maximum spanning forest (kernel_forest.cuh).
// The lock-free union-find, the degree tally, the three kinds of edge list, an entry as an edge (the cut, the range check and its
// tally), and the order-preserving image of a value.  Part of libselhip.so; included by selection_kernels.hip only, in front of those three.
// The memory model behind cl_load / cl_min / cl_unite is argued at the head of kernel_cluster.cuh.
#pragma once

namespace {

constexpr int kClusterMaxBlocks = 4096;        // edge kernels: 256 CUs x 16 blocks of 4 waves; beyond it the lanes stride

// what an edge kernel found wrong with its list: entries with a vertex outside [0, n), and the smallest index of one (~0 = none)
struct ClusterBad { u64 count; u64 index; };

__device__ __forceinline__ int cl_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ int cl_min(int* p, int v) { return __hip_atomic_fetch_min(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root above x as far as this lane can see it.  parent[y] < y for every y that is not a root, so x falls strictly in every
// iteration: at most x steps, and nothing is waited for.  A chain of two links or more is shortened: parent[x0] = min(parent[x0], root)
// by an atomic minimum -- the root is an ancestor of x0, and an ancestor that is <= the current parent is always a valid parent
__device__ __forceinline__ int cl_find(int* parent, int x0) {
    int x = x0, p = cl_load(parent + x), hops = 0;
    while (p != x) { x = p; p = cl_load(parent + x); ++hops; }
    if (hops > 1) (void)cl_min(parent + x0, x);
    return x;
}

// unite the trees of u and v.  With a, b the two roots found: hook the larger (hi) under the smaller (lo) by
// old = atomic_min(&parent[hi], lo).  old == hi: hi was still a root and hangs under lo now -- done.  Otherwise somebody hooked hi first,
// under old < hi; parent[hi] is min(old, lo) now, both old and lo are vertices of hi's component, and whichever of them hi no longer
// (or never) points to still has to meet the other: go on with the pair (old, lo).
// Termination: max(a, b) falls strictly in every iteration -- the next pair is (root above old, root above lo) with old < hi, lo < hi and
// roots never above their vertices -- so the loop ends after at most n steps, whatever the other lanes do; it never waits for them.
__device__ __forceinline__ void cl_unite(int* parent, int u, int v) {
    int a = cl_find(parent, u), b = cl_find(parent, v);
    while (a != b) {
        const int hi = a > b ? a : b, lo = a > b ? b : a;
        const int old = cl_min(parent + hi, lo);
        if (old == hi || old == lo) break;
        a = cl_find(parent, old);
        b = cl_find(parent, lo);
    }
}

// degree[x] += 1 for every lane with ok.  The lists of the passes come in runs of one query row (a wave of the count or join kernels
// appends a row's partners together), so a wave's 64 records name a few distinct i and 64 atomic adds to ONE address serialise at the
// memory side: the lanes that share the vertex of the first lane still to add do it as one add of their number, twice over; whoever is
// left adds for itself (consecutive partners: one coalesced instruction).  Measured on the dense-sharing set of 4 096 genomes, 8.4e6
// records: see DESIGN.md section 21.  Integer adds in any grouping give the same sums.  (todo is wave-uniform: the loop branches on SGPRs.)
__device__ __forceinline__ void cl_degree_add(int* __restrict__ degree, int x, bool ok) {
    const int lane = (int)__lane_id();
    u64 todo = __ballot(ok);
    for (int round = 0; round < 2 && todo; ++round) {
        const int leader = __ffsll((long long)todo) - 1;
        const int lx = __builtin_amdgcn_readlane(x, leader);
        const u64 same = __ballot(ok && x == lx) & todo;
        if (lane == leader) atomicAdd(degree + lx, (int)__popcll(same));
        todo &= ~same;
    }
    if (ok && ((todo >> lane) & 1ull)) atomicAdd(degree + x, 1);
}

// the three kinds of list.  edge(e) gives entry e as (u, v, value) and whether it is an edge of the graph at all:
//   a caller's entries {x, y}, all of them edges, at value 1.0;
//   the same with values[e], or 1.0 where there are none (a struct of its own: the plain list's kernels take one pointer);
//   a pass's records {i, k, value}, edges where value >= min_value
struct GraphPairList {
    const selhip_int2_t* p;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v, double* value) const { const selhip_int2_t r = p[e]; *u = r.x; *v = r.y; *value = 1.0; return true; }
};
struct GraphValuedPairList {
    const selhip_int2_t* p;
    const double* values;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v, double* value) const {
        const selhip_int2_t r = p[e]; *u = r.x; *v = r.y;
        *value = values ? values[e] : 1.0;
        return true;
    }
};
struct GraphRecordList {
    const selhip_pair_t* p;                     // 16-byte records, 16-byte aligned: one dwordx4 per lane, a wave reads 1 KiB in a row
    double min_value;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v, double* value) const {
        const uint4 w = reinterpret_cast<const uint4*>(p)[e];
        *u = (int)w.x; *v = (int)w.y;
        *value = __hiloint2double((int)w.w, (int)w.z);
        return *value >= min_value;             // NaN never passes, -inf takes everything
    }
};

// entry e of a list as an edge of the graph: false for one below the cut and for one with a vertex outside [0, n), which is tallied
// in *bad -- kBadMayBeNull: where the caller passes it (one launch per call does) -- and must touch nothing
template <bool kBadMayBeNull, class List>
__device__ __forceinline__ bool graph_edge(const List& list, u64 e, int n, int* u, int* v, double* value, ClusterBad* __restrict__ bad) {
    if (!list.edge(e, u, v, value)) return false;
    if ((uint32_t)*u >= (uint32_t)n || (uint32_t)*v >= (uint32_t)n) {
        if (!kBadMayBeNull || bad) { atomicAdd(&bad->count, 1ull); atomicMin(&bad->index, e); }
        return false;
    }
    return true;
}

// the order-preserving integer image of a value that is no NaN: a > b in f64 <=> image(a) > image(b), and -0.0 == +0.0 have one
// image (canonicalised first).  Every image is > 0, so 0 is "no edge yet".  graph_value is its inverse
__device__ __forceinline__ u64 graph_image(double v) {
    if (v == 0.0) v = 0.0;                      // -0.0 -> +0.0
    const u64 b = (u64)__double_as_longlong(v);
    return (b >> 63) ? ~b : b | 0x8000000000000000ull;
}
__device__ __forceinline__ double graph_value(u64 image) {
    return __longlong_as_double((long long)((image >> 63) ? image & 0x7FFFFFFFFFFFFFFFull : ~image));
}

}  // namespace

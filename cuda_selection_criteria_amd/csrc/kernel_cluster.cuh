// kernel_cluster.cuh -- single-linkage clusters of a record list: the connected components of the graph whose edges are the records
// (selhip_components, selhip_ctx_cluster; host side in host_cluster.hpp).  Part of libselhip.so; included by selection_kernels.hip only.
//
// A lock-free union-find over parent[n] with the invariant parent[x] <= x (a root is its own parent), so the root of a tree is its
// smallest vertex and, once every edge is in, the smallest vertex of the component: the labels are a pure function of the edge SET,
// whatever order the lanes ran in.  The launches:
//   cluster_init_kernel       parent[g] = g, the tallies cleared
//   cluster_edges_kernel      one lane per record, grid-stride: validate, [threshold], [degree tally], unite(u, v)
//   cluster_flatten_kernel    label[g] = root(g) into an array of its own, members per root, root flags
//   (rocprim::exclusive_scan of the root flags: the dense ids, numbered by ascending label)
//   cluster_assign_kernel     cluster[g], cluster_size[c], and the representative's key by a 64-bit atomic maximum
//   cluster_rep_kernel        cluster_rep[c] decoded from the key
//   cluster_singletons_kernel the whole answer of a list without edges, in the one launch
//
// Memory model (MI355X: the vector L1 is per CU and never refreshed by another CU's stores, the L2s of the eight XCDs are not coherent
// with each other).  Inside cluster_edges_kernel parent[] is shared by every lane of the grid, so there
//   * every WRITE to it is an agent-scope atomic minimum (cl_min), performed at the memory side: no store can be lost or linger in a cache;
//   * every READ of it is an agent-scope relaxed atomic load (cl_load: global_load ... sc1, served beyond L1).  A value read may still
//     be old by the time it is used.  That is harmless by construction: parent[x] only ever falls, every value it has held is a vertex of
//     x's component that stays reachable from x (see cl_unite), so an old value is an ancestor all the same -- the walk just takes more steps --
//     and a hook that acted on an old root fails its compare (old != hi) and is retried on what it read.
// No loop waits for the progress of another lane, wave or block: no spin, no flag, no grid barrier, no cooperative launch.  Every loop
// is bounded by a quantity that falls strictly in each of the lane's own iterations.  Visibility BETWEEN the launches comes from the
// kernel boundary alone; behind it the other kernels read parent[] / label[] with plain loads.  The tallies (degrees, members) are
// integer atomic adds without a return value and the representative an integer atomic maximum: order-independent, so every output is
// bit-reproducible.
#pragma once

namespace {

constexpr int kClusterMaxBlocks = 4096;        // edge kernel: 256 CUs x 16 blocks of 4 waves; beyond it the lanes stride

// what the edge kernel found wrong with its list: entries with a vertex outside [0, n), and the smallest index of one (~0 = none)
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

__global__ void __launch_bounds__(kBlock)
cluster_init_kernel(int* __restrict__ parent, int* __restrict__ degree, int* __restrict__ members, uint32_t* __restrict__ flag,
                    u64* __restrict__ key, long long n, ClusterBad* __restrict__ bad) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        parent[g] = (int)g;
        if (degree) degree[g] = 0;
        if (members) members[g] = 0;
        if (key) key[g] = 0;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (flag) flag[n] = 0;                  // one slot past the last vertex: the scan's total lands there
        bad->count = 0; bad->index = ~0ull;
    }
}

// the two kinds of list: a caller's entries {x, y}, all of them edges, and a pass's records {i, k, value}, edges where value >= min_value
struct ClusterPairList {
    const selhip_int2_t* p;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v) const { const selhip_int2_t r = p[e]; *u = r.x; *v = r.y; return true; }
};
struct ClusterRecordList {
    const selhip_pair_t* p;                     // 16-byte records, 16-byte aligned: one dwordx4 per lane, a wave reads 1 KiB in a row
    double min_value;
    __device__ __forceinline__ bool edge(u64 e, int* u, int* v) const {
        const uint4 w = reinterpret_cast<const uint4*>(p)[e];
        *u = (int)w.x; *v = (int)w.y;
        return __hiloint2double((int)w.w, (int)w.z) >= min_value;      // NaN never passes, -inf takes everything
    }
};

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

// one lane per record, grid-stride with a 64-bit index.  degree (may be null): every edge adds one to both of its vertices -- records are
// counted, not distinct partners.  An entry with a vertex outside [0, n) is tallied in *bad and touches nothing else
template <class List>
__global__ void __launch_bounds__(kBlock)
cluster_edges_kernel(const List list, u64 n_edges, int n, int* __restrict__ parent, int* __restrict__ degree, ClusterBad* __restrict__ bad) {
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        bool ok = list.edge(e, &u, &v);
        if (ok && ((uint32_t)u >= (uint32_t)n || (uint32_t)v >= (uint32_t)n)) {
            atomicAdd(&bad->count, 1ull);
            atomicMin(&bad->index, e);
            ok = false;
        }
        if (degree) { cl_degree_add(degree, u, ok); cl_degree_add(degree, v, ok); }
        if (ok && u != v) cl_unite(parent, u, v);
    }
}

// behind the edge kernel's end every parent[] value is final and visible: plain loads.  members / flag may be null
__global__ void __launch_bounds__(kBlock)
cluster_flatten_kernel(const int* __restrict__ parent, long long n, int* __restrict__ label, int* __restrict__ members, uint32_t* __restrict__ flag) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        int r = (int)g, p = parent[r];
        while (p != r) { r = p; p = parent[r]; }            // r falls strictly: at most g steps
        label[g] = r;
        if (members) atomicAdd(members + r, 1);
        if (flag) flag[g] = r == (int)g ? 1u : 0u;
    }
}

// the representative's key: its maximum over a cluster's members picks
//   SELHIP_REP_MAX_DEGREE  (degree, reversed rank): the most records, ties to the smaller rank
//   SELHIP_REP_MIN_RANK    reversed rank;   SELHIP_REP_MAX_RANK  rank
__device__ __forceinline__ u64 cluster_rep_key(int rule, int g, int deg) {
    const u64 rev = 0xFFFFFFFFull - (u64)(uint32_t)g;
    return rule == SELHIP_REP_MAX_DEGREE ? ((u64)(uint32_t)deg << 32) | rev : rule == SELHIP_REP_MIN_RANK ? rev : (u64)(uint32_t)g;
}
__device__ __forceinline__ int cluster_rep_of(int rule, u64 key) {
    return rule == SELHIP_REP_MAX_RANK ? (int)(uint32_t)key : (int)(0xFFFFFFFFu - (uint32_t)key);
}

// ids[r] = the exclusive scan of the root flags: the dense id of root r.  cluster / cluster_size / key may be null
__global__ void __launch_bounds__(kBlock)
cluster_assign_kernel(const int* __restrict__ label, const int* __restrict__ members, const int* __restrict__ degree,
                      const uint32_t* __restrict__ ids, long long n, int rule, int* __restrict__ cluster, int* __restrict__ cluster_size,
                      u64* __restrict__ key) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        const int r = label[g];
        const uint32_t c = ids[r];
        if (cluster) cluster[g] = (int)c;
        if (cluster_size && r == (int)g) cluster_size[c] = members[g];
        if (key) atomicMax(key + c, cluster_rep_key(rule, (int)g, degree ? degree[g] : 0));
    }
}

// ids[n] = the number of clusters C: entries [0, C) of cluster_rep are written
__global__ void __launch_bounds__(kBlock)
cluster_rep_kernel(const u64* __restrict__ key, const uint32_t* __restrict__ ids, long long n, int rule, int* __restrict__ cluster_rep) {
    const long long n_clusters = (long long)ids[n], stride = (long long)gridDim.x * kBlock;
    for (long long c = (long long)blockIdx.x * kBlock + threadIdx.x; c < n_clusters; c += stride) cluster_rep[c] = cluster_rep_of(rule, key[c]);
}

// a list without edges: n singletons, each its own label, cluster and representative, with no record.  Every pointer may be null
__global__ void __launch_bounds__(kBlock)
cluster_singletons_kernel(long long n, int* __restrict__ label, int* __restrict__ cluster, int* __restrict__ degree,
                          int* __restrict__ cluster_size, int* __restrict__ cluster_rep) {
    const long long stride = (long long)gridDim.x * kBlock;
    for (long long g = (long long)blockIdx.x * kBlock + threadIdx.x; g < n; g += stride) {
        if (label) label[g] = (int)g;
        if (cluster) cluster[g] = (int)g;
        if (degree) degree[g] = 0;
        if (cluster_size) cluster_size[g] = 1;
        if (cluster_rep) cluster_rep[g] = (int)g;
    }
}

}  // namespace

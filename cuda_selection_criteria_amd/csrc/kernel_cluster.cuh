// kernel_cluster.cuh -- single-linkage clusters of a record list: the connected components of the graph whose edges are the records
// (selhip_components, selhip_ctx_cluster; host side in host_cluster.hpp).  Part of libselhip.so; included by selection_kernels.hip only,
// behind kernel_graph.cuh, where the union-find itself (cl_load, cl_min, cl_find, cl_unite), cl_degree_add, ClusterBad and the lists live.
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

// one lane per record, grid-stride with a 64-bit index (List: kernel_graph.cuh's; the value is not looked at).  degree (may be null):
// every edge adds one to both of its vertices -- records are counted, not distinct partners.  An entry with a vertex outside [0, n) is
// tallied in *bad and touches nothing else
template <class List>
__global__ void __launch_bounds__(kBlock)
cluster_edges_kernel(const List list, u64 n_edges, int n, int* __restrict__ parent, int* __restrict__ degree, ClusterBad* __restrict__ bad) {
    const u64 stride = (u64)gridDim.x * kBlock;
    for (u64 e = (u64)blockIdx.x * kBlock + threadIdx.x; e < n_edges; e += stride) {
        int u, v;
        double value;
        const bool ok = graph_edge<false>(list, e, n, &u, &v, &value, bad);
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

// kmu_components.hip -- connected components over an edge list, on the device (kmu_components, kmu_components_knn; the semantics
// are in include/kmu.h).  One implementation, a template over "edge e -> (u, v, counts)": records of uint32 words with an optional
// weight word, or the neighbour lists of a kmu_sig_knn self-join.  label_out is the parent array of a lock-free union-find.
//
//  k_cc_init     parent[v] = v.
//  k_cc_hook     one lane per edge, grid-stride.  An edge that does not count, a self loop and an edge with an endpoint >= n_nodes
//                are dropped before parent is touched.  The lane finds the roots of both ends (cc_find: relaxed agent-scope
//                atomic loads, path halving by atomicMin), leaves if they are equal, and otherwise hooks the LARGER root under the
//                SMALLER by atomicCAS(parent[larger], larger, smaller).  A CAS that fails has seen the value some other lane put
//                there: the lane goes on with (that value, smaller).  A retry therefore follows progress of another lane and no lane
//                waits for one.
//                Invariant: parent[v] <= v, and an entry only ever decreases (a hook replaces r by something smaller, a halving is
//                an atomicMin).  A walk towards the root is strictly decreasing, so it ends; a root is the smallest node of its tree;
//                when the kernel is over every edge that counts has both ends in one tree.  The root of a component is therefore its
//                smallest node, whichever lane won which race: the labels do not depend on the order of the edges or of the lanes.
//  k_cc_flatten  label[v] = root(v), in place (no hook runs any more: a root stays a root, and every value a concurrent walk
//                reads is an ancestor); root flags for the scan and zeros for the sizes.
//  device_scan_u32 over the root flags: rank[r] = the number of roots below r, rank[n_nodes] = the number of components.
//  k_cc_number   cluster[v] = rank[label[v]]; integer atomicAdds into size[cluster], the lanes of a wave that share a cluster adding once
//                together (a few rounds, then lane by lane); (cluster, node) entries.
//  radix_sort_pairs_passes on the cluster number (the bytes that n_nodes - 1 can reach: the number of components stays on the device,
//                and n_components <= n_nodes); the sort is stable, so the nodes of a cluster stay ascending.
// Each step behind k_cc_flatten runs only when an output that needs it was asked for.  Integer arithmetic throughout.
#include <algorithm>

#include "kmu_sort.h"

namespace kmu {

// edge e of an array of records: words 0 and 1 are the ends, word weight_at (when not 0) decides whether it counts
struct CcRecords {
    const uint32_t *edges;
    uint32_t stride, weight_at, min_weight;
    __device__ __forceinline__ bool get(uint64_t e, uint32_t &u, uint32_t &v) const {
        const uint32_t *r = edges + e * stride; // 64-bit: n_edges * stride may pass 2^32
        u = r[0];
        v = r[1];
        return weight_at == 0 || r[weight_at] >= min_weight;
    }
};

// edge e = i * k + j of the lists of a self-join: (i, idx[e]), counting iff eq[e] >= min_eq
struct CcKnn {
    const uint32_t *idx;
    const uint16_t *eq;
    uint32_t k, min_eq;
    __device__ __forceinline__ bool get(uint64_t e, uint32_t &u, uint32_t &v) const {
        u = (uint32_t) (e / k);
        v = idx[e];
        return min_eq == 0 || (uint32_t) eq[e] >= min_eq;
    }
};

static constexpr int CC_SIZE_ROUNDS = 4; // k_cc_number: rounds in which the lanes of one cluster add to its size together

__device__ __forceinline__ uint32_t cc_load(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// the root of v as of some moment during the call; v < n_nodes.  Path halving: a node whose parent is no root is moved to its
// grandparent (atomicMin: an entry never rises, whatever other lanes do to it meanwhile).
__device__ __forceinline__ uint32_t cc_find(uint32_t *parent, uint32_t v) {
    uint32_t p = cc_load(parent + v);
    while (p != v) {
        const uint32_t g = cc_load(parent + p);
        if (g == p) return p;
        atomicMin(parent + v, g);
        v = p;
        p = g;
    }
    return v;
}

__global__ void __launch_bounds__(256) k_cc_init(uint32_t *parent, uint32_t n_nodes) {
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_nodes; v += (uint64_t) gridDim.x * blockDim.x)
        parent[v] = (uint32_t) v;
}

template <class E> __global__ void __launch_bounds__(256) k_cc_hook(E edges, uint64_t n_edges, uint32_t *parent, uint32_t n_nodes) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n_edges; e += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t u, v;
        if (!edges.get(e, u, v) || u == v || u >= n_nodes || v >= n_nodes) continue;
        for (;;) {
            u = cc_find(parent, u);
            v = cc_find(parent, v);
            if (u == v) break; // one tree already: the edge leaves without an atomic on a root
            const uint32_t hi = max(u, v), lo = min(u, v);
            const uint32_t seen = atomicCAS(parent + hi, hi, lo);
            if (seen == hi) break;
            u = seen; // another lane hooked hi under `seen` (< hi): what is left to join is (seen, lo)
            v = lo;
        }
    }
}

__global__ void __launch_bounds__(256) k_cc_flatten(uint32_t *parent, uint32_t n_nodes, uint32_t *is_root, uint32_t *size) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t v = (uint32_t) i;
        uint32_t r = v, p = cc_load(parent + r);
        while (p != r) {
            r = p;
            p = cc_load(parent + r);
        }
        if (r != v) __hip_atomic_store(parent + v, r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (is_root) is_root[v] = r == v;
        if (size) size[v] = 0;
    }
}

__global__ void __launch_bounds__(256) k_cc_number(const uint32_t *label, const uint64_t *rank, uint32_t n_nodes, uint32_t *cluster,
                                                   uint32_t *size, uint64_t *keys, uint32_t *vals) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_nodes; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t c = (uint32_t) rank[label[i]]; // label < n_nodes, rank of a root < n_components <= n_nodes
        if (cluster) cluster[i] = c;
        if (size) {
            // A million adds to the one counter of a giant cluster run one after the other (measured: 11 ms of a 16 ms call over 10^6
            // nodes).  So a few rounds first, in each of which the lanes that share the cluster of the first lane left add once
            // together; what is left after that -- a wave of many small clusters -- adds lane by lane.
            uint64_t todo = __ballot(1);
            bool mine = true;
            for (int round = 0; round < CC_SIZE_ROUNDS && todo; round++) {
                const int lead = __ffsll((unsigned long long) todo) - 1;
                const uint32_t c0 = (uint32_t) __shfl((int) c, lead, 64);
                const uint64_t same = __ballot(mine && c == c0);
                if (lane_id() == lead) atomicAdd(size + c0, (uint32_t) __popcll(same));
                if (c == c0) mine = false;
                todo &= ~same;
            }
            if (mine) atomicAdd(size + c, 1u);
        }
        if (keys) {
            keys[i] = c;
            vals[i] = (uint32_t) i;
        }
    }
}

// the common part of both entry points: `edges` reads device memory (staged by the caller), the outputs are the caller's
template <class E>
static int components_run(kmu_ctx *ctx, uint32_t n_nodes, const E &edges, uint64_t n_edges, int mem, uint32_t *label_out,
                          uint32_t *cluster_out, uint32_t *size_out, uint32_t *members_out, uint32_t *n_components_out) {
    uint32_t *label, *cluster, *size;
    KMU_TRY(place_output(ctx, "cc.label", label_out, n_nodes, mem, &label));
    KMU_TRY(place_output(ctx, "cc.cluster", cluster_out, n_nodes, mem, &cluster));
    KMU_TRY(place_output(ctx, "cc.size", size_out, n_nodes, mem, &size));
    const bool numbered = cluster_out || size_out || members_out;
    const bool ranked = numbered || n_components_out;
    uint32_t *is_root = nullptr, *v0 = nullptr, *v1 = nullptr;
    uint64_t *rank = nullptr, *k0 = nullptr, *k1 = nullptr;
    if (ranked) {
        KMU_TRY(dev_array(ctx, "cc.isroot", n_nodes, &is_root));
        KMU_TRY(dev_array(ctx, "cc.rank", (size_t) n_nodes + 1, &rank));
    }
    if (members_out) {
        KMU_TRY(dev_array(ctx, "cc.keys0", n_nodes, &k0));
        KMU_TRY(dev_array(ctx, "cc.vals0", n_nodes, &v0));
        KMU_TRY(dev_array(ctx, "cc.keys1", n_nodes, &k1));
        KMU_TRY(dev_array(ctx, "cc.vals1", n_nodes, &v1));
    }

    const int node_grid = grid_for(ctx, n_nodes, 256); // about 2048 workgroups at most, the rest by grid stride
    KMU_TRY(launch(ctx, "k_cc_init", k_cc_init, dim3(node_grid), dim3(256), 0, label, n_nodes));
    if (n_edges) KMU_TRY(launch(ctx, "k_cc_hook", k_cc_hook<E>, dim3(grid_for(ctx, n_edges, 256)), dim3(256), 0, edges, n_edges, label, n_nodes));
    KMU_TRY(launch(ctx, "k_cc_flatten", k_cc_flatten, dim3(node_grid), dim3(256), 0, label, n_nodes, is_root, size));
    if (ranked) KMU_TRY(device_scan_u32(ctx, is_root, n_nodes, rank));
    if (numbered) KMU_TRY(launch(ctx, "k_cc_number", k_cc_number, dim3(node_grid), dim3(256), 0, label, rank, n_nodes, cluster, size, k0, v0));
    if (members_out) {
        KMU_TRY(radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n_nodes, radix_id_passes(n_nodes), nullptr));
        KMU_TRY(copy_out(ctx, members_out, v0, (size_t) n_nodes * 4, mem));
    }
    KMU_TRY(bring_output(ctx, label_out, label, n_nodes, mem));
    KMU_TRY(bring_output(ctx, cluster_out, cluster, n_nodes, mem));
    KMU_TRY(bring_output(ctx, size_out, size, n_nodes, mem));
    if (n_components_out) { // the one synchronisation of a device call: the count crosses to the host
        uint64_t total = 0;
        KMU_TRY(read_back(ctx, {{&total, rank + n_nodes}}));
        *n_components_out = (uint32_t) total;
    }
    return finish_call(ctx, mem);
}

static int cc_check_common(kmu_ctx *ctx, uint32_t n_nodes, int mem, const uint32_t *label_out) {
    if (!ctx || !label_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    KMU_TRY(check_mem(ctx, mem));
    if (n_nodes == 0xFFFFFFFFu) return fail(ctx, KMU_E_UNSUPPORTED, "n_nodes = 2^32 - 1: node numbers must stay below KMU_KNN_NONE");
    return KMU_OK;
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_components(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *edges, uint64_t n_edges, uint32_t stride,
                              uint32_t weight_at, uint32_t min_weight, int mem, uint32_t *label_out, uint32_t *cluster_out,
                              uint32_t *size_out, uint32_t *members_out, uint32_t *n_components_out) {
    if (!ctx || !label_out || (!edges && n_edges > 0)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (stride < 2) return fail(ctx, KMU_E_BAD_ARG, "stride = %u: a record holds at least its two ends", stride);
    if (weight_at == 1 || weight_at >= stride)
        return fail(ctx, KMU_E_BAD_ARG, "weight_at = %u: must be 0 or a word behind the ends of a record of %u words", weight_at, stride);
    KMU_TRY(cc_check_common(ctx, n_nodes, mem, label_out));
    if (n_components_out) *n_components_out = 0;
    if (n_nodes == 0) return KMU_OK;
    if (n_edges > SIZE_MAX / 4 / stride) return fail(ctx, KMU_E_UNSUPPORTED, "%llu records of %u words", (unsigned long long) n_edges, stride);
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *d_edges;
    KMU_TRY(stage_to_device(ctx, "cc.edges", edges, (size_t) n_edges * stride, mem, &d_edges));
    const CcRecords rec{d_edges, stride, weight_at, min_weight};
    return components_run(ctx, n_nodes, rec, n_edges, mem, label_out, cluster_out, size_out, members_out, n_components_out);
}

extern "C" int kmu_components_knn(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *idx, const uint16_t *eq, uint32_t k, uint32_t min_eq,
                                  int mem, uint32_t *label_out, uint32_t *cluster_out, uint32_t *size_out, uint32_t *members_out,
                                  uint32_t *n_components_out) {
    if (!ctx || !label_out || (!idx && n_nodes > 0)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (k == 0 && n_nodes > 0) return fail(ctx, KMU_E_BAD_ARG, "k = 0: lists without entries");
    if (!eq && min_eq > 0) return fail(ctx, KMU_E_BAD_ARG, "min_eq = %u without eq", min_eq);
    KMU_TRY(cc_check_common(ctx, n_nodes, mem, label_out));
    if (n_components_out) *n_components_out = 0;
    if (n_nodes == 0) return KMU_OK;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_edges = (uint64_t) n_nodes * k;
    const uint32_t *d_idx;
    const uint16_t *d_eq;
    KMU_TRY(stage_to_device(ctx, "cc.edges", idx, (size_t) n_edges, mem, &d_idx));
    KMU_TRY(stage_to_device(ctx, "cc.eq", eq, (size_t) n_edges, mem, &d_eq));
    const CcKnn lists{d_idx, d_eq, k, eq ? min_eq : 0u};
    return components_run(ctx, n_nodes, lists, n_edges, mem, label_out, cluster_out, size_out, members_out, n_components_out);
}

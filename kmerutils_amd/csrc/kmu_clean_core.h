// kmu_clean_core.h -- the arithmetic of string graph cleaning: which arcs the device may use, the mate search, the walk of a tip, the
// spare rule of a junction, the walk of a bubble's branch and the choice of the branch that loses; for the device and for a host
// compiler alike (tests/cpp/sim_clean.cpp drives these functions over simulated lanes; the contract is in include/kmu.h).
//
// deg[v] is the number of surviving arcs of out(v), so in(v) = deg[v ^ 1].  sole[v] is the smallest `to` over the surviving arcs of
// out(v): THE successor of v where deg[v] == 1, and read nowhere else.  Every walk is bounded by its limit (at most KMU_SG_CLEAN_MAX
// dependent loads), whatever the graph looks like.
#pragma once

#include <stdint.h>

#include "kmu_sg_core.h"

#ifdef __HIPCC__
#define KMU_CL_HD __host__ __device__ __forceinline__
#else
#define KMU_CL_HD inline
#endif

namespace kmu {

static_assert(sizeof(kmu_sg_clean_params) == 16 && sizeof(kmu_sg_clean_stats) == 64, "the records of include/kmu.h");

KMU_CL_HD bool cl_survives(const kmu_sg_arc &a) { return a.flags == 0u; }
// what can be said of a surviving arc before it is used as an index
KMU_CL_HD bool cl_arc_ok(const kmu_sg_arc &a, uint32_t n_reads) {
    const uint64_t n_v = 2ull * n_reads;
    return a.from < n_v && a.to < n_v && (a.from >> 1) != (a.to >> 1);
}
// does the surviving arc x = v -> w have a surviving arc w^1 -> v^1 of the same rec (x has passed cl_arc_ok; the slice is only
// known to be sorted by `from`, so it is walked)
KMU_CL_HD bool cl_has_mate(const kmu_sg_arc *arcs, uint64_t n, const kmu_sg_arc &x) {
    const uint32_t mf = x.to ^ 1u, mt = x.from ^ 1u;
    for (uint64_t i = sg_lower_from(arcs, n, mf); i < n && arcs[i].from == mf; i++)
        if (arcs[i].to == mt && arcs[i].rec == x.rec && cl_survives(arcs[i])) return true;
    return false;
}
KMU_CL_HD uint32_t cl_in(const uint32_t *deg, uint32_t v) { return deg[v ^ 1u]; }

// ---- tips ---------------------------------------------------------------------------------------------------------------------------
struct ClTip {
    uint32_t cnt, last, junction; // cnt == 0: v0 starts no candidate tip
};
// the walk of the contract from v0 with the limit T >= 1
KMU_CL_HD ClTip cl_tip_walk(const uint32_t *deg, const uint32_t *sole, uint32_t v0, uint32_t T) {
    ClTip t{0u, KMU_SG_NONE, KMU_SG_NONE};
    if (T == 0u || cl_in(deg, v0) != 0u || deg[v0] != 1u) return t;
    uint32_t v = v0;
    for (uint32_t i = 0; i < T; i++) { // on arriving at w from v(i) the reads so far are i + 1 <= T
        const uint32_t w = sole[v];
        if (cl_in(deg, w) >= 2u) {
            t.cnt = i + 1u;
            t.last = v;
            t.junction = w;
            return t;
        }
        if (deg[w] != 1u) return t; // a line that ends, or a stem before a fork
        v = w;
    }
    return t; // too long
}
// the candidate tip end that junction w spares (tipcnt[u]: the reads of the candidate whose last vertex is u, else 0), or
// KMU_SG_NONE where some in-neighbour of w is no candidate tip end or w is no junction
KMU_CL_HD uint32_t cl_spared(const kmu_sg_arc *arcs, uint64_t n, const uint32_t *deg, const uint32_t *tipcnt, uint32_t w) {
    if (cl_in(deg, w) < 2u) return KMU_SG_NONE;
    uint32_t best = KMU_SG_NONE, best_cnt = 0u;
    const uint32_t m = w ^ 1u;
    for (uint64_t i = sg_lower_from(arcs, n, m); i < n && arcs[i].from == m; i++) {
        if (!cl_survives(arcs[i])) continue;
        const uint32_t u = arcs[i].to ^ 1u, c = tipcnt[u];
        if (c == 0u) return KMU_SG_NONE;
        if (c > best_cnt || (c == best_cnt && u < best)) {
            best = u;
            best_cnt = c;
        }
    }
    return best;
}

// ---- bubbles ------------------------------------------------------------------------------------------------------------------------
struct ClBranch {
    uint32_t k, t, min_read; // k == 0: no branch
};
// the branch that begins at a1, with at most B interior vertices
KMU_CL_HD ClBranch cl_branch(const uint32_t *deg, const uint32_t *sole, uint32_t a1, uint32_t B) {
    ClBranch b{0u, KMU_SG_NONE, KMU_SG_NONE};
    uint32_t x = a1, min_read = KMU_SG_NONE;
    for (uint32_t k = 1; k <= B; k++) { // x is the k-th vertex: interior iff in = out = 1
        if (cl_in(deg, x) != 1u || deg[x] != 1u) return b;
        if ((x >> 1) < min_read) min_read = x >> 1;
        const uint32_t y = sole[x];
        if (cl_in(deg, y) == 2u) {
            b.k = k;
            b.t = y;
            b.min_read = min_read;
            return b;
        }
        x = y;
    }
    return b;
}
// the targets of the two surviving arcs of s (deg[s] == 2), in list order
struct ClPair {
    uint32_t a, b, found;
};
KMU_CL_HD ClPair cl_two_arcs(const kmu_sg_arc *arcs, uint64_t n, uint32_t s) {
    uint32_t a = KMU_SG_NONE, b = KMU_SG_NONE, found = 0;
    for (uint64_t i = sg_lower_from(arcs, n, s); i < n && arcs[i].from == s; i++) {
        if (!cl_survives(arcs[i])) continue;
        const uint32_t to = arcs[i].to;
        a = found == 0u ? to : a; // (selects, not stores through an index: the pair stays in registers)
        b = found == 1u ? to : b;
        found++;
    }
    return ClPair{a, b, found};
}
struct ClBubble {
    uint32_t k, t, first; // k == 0: s is the source of no bubble; else the loser's interior is `first` and k - 1 successors
};
KMU_CL_HD ClBubble cl_bubble(const kmu_sg_arc *arcs, uint64_t n, const uint32_t *deg, const uint32_t *sole, uint32_t s, uint32_t B) {
    ClBubble r{0u, KMU_SG_NONE, KMU_SG_NONE};
    if (B == 0u || deg[s] != 2u) return r;
    const ClPair p = cl_two_arcs(arcs, n, s);
    if (p.found != 2u) return r; // (never: deg counted the same arcs)
    const uint32_t a = p.a, b = p.b;
    const ClBranch x = cl_branch(deg, sole, a, B), y = cl_branch(deg, sole, b, B);
    if (x.k == 0u || y.k == 0u || x.t != y.t || (x.t >> 1) == (s >> 1)) return r;
    const bool x_loses = x.k != y.k ? x.k < y.k : x.min_read > y.min_read;
    r.k = x_loses ? x.k : y.k;
    r.t = x.t;
    r.first = x_loses ? a : b;
    return r;
}
// a bubble is counted once, at the smaller of s and t ^ 1
KMU_CL_HD bool cl_bubble_counts(uint32_t s, uint32_t t) { return s < (t ^ 1u); }

// ---- finish -------------------------------------------------------------------------------------------------------------------------
// the flag an arc gains from the flags of its two reads: `bit` (an arc flag) where either read carries it (the read flags have the
// same values)
KMU_CL_HD uint32_t cl_arc_flag(uint32_t flags_from, uint32_t flags_to, uint32_t bit) { return ((flags_from | flags_to) & bit) ? bit : 0u; }
KMU_CL_HD uint32_t cl_unique(const kmu_sg_arc &a, const uint32_t *deg) { return cl_survives(a) && deg[a.from] == 1u && cl_in(deg, a.to) == 1u; }

} // namespace kmu

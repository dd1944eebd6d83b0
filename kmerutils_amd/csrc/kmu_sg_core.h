// kmu_sg_core.h -- the arithmetic of the string graph: which records the device may touch, the class of a record, the two arcs of a
// dovetail, the searches over the sorted arc list, a vertex's L and first, and the reduction rule with the marking of a run; for the
// device and for a host compiler alike (tests/cpp/sim_string_graph.cpp drives these functions over 64 simulated lanes; the contract
// is in include/kmu.h).
//
// The arc list is sorted by (from, to, rec), so out(v) is one slice, the arcs v -> x of it are one RUN inside the slice, and the
// first arc of the smallest len in a slice is first(v) under (len, to, rec).
#pragma once

#include <stdint.h>

#include "../../include/kmu.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_SG_HD __host__ __device__ __forceinline__
#else
#define KMU_SG_HD inline
#endif

namespace kmu {

static_assert(sizeof(kmu_sg_arc) == 32 && sizeof(kmu_sg_read) == 16 && sizeof(kmu_sg_params) == 24, "the records of include/kmu.h");

// what can be said of a record before any length is fetched: its reads exist, the strand is one, no start is above its end
KMU_SG_HD bool sg_record_ok(const kmu_chain &c, uint32_t n_reads) {
    return c.read_a < n_reads && c.read_b < n_reads && c.strand <= 1u && c.a_start <= c.a_end && c.b_start <= c.b_end;
}
// and with the lengths of its two reads: they fit 32 bits and hold the ends
KMU_SG_HD bool sg_lengths_ok(const kmu_chain &c, uint64_t la, uint64_t lb) {
    return la <= 0xFFFFFFFFull && lb <= 0xFFFFFFFFull && c.a_end <= la && c.b_end <= lb;
}

// the four overhangs of a record, b in a's orientation
struct SgHangs {
    uint64_t aL, aR, bL, bR;
};
KMU_SG_HD SgHangs sg_hangs(const kmu_chain &c, uint64_t la, uint64_t lb) {
    SgHangs h;
    h.aL = c.a_start;
    h.aR = la - c.a_end;
    h.bL = c.strand ? lb - c.b_end : (uint64_t) c.b_start;
    h.bR = c.strand ? (uint64_t) c.b_start : lb - c.b_end;
    return h;
}

// the class of a record that sg_record_ok and sg_lengths_ok pass; aln == nullptr: no identity test
KMU_SG_HD uint32_t sg_class(const kmu_chain &c, uint64_t la, uint64_t lb, const kmu_chain_aln *aln, const kmu_sg_params &p) {
    if (c.read_a >= c.read_b) return KMU_SG_SKIP;
    const uint64_t oa = c.a_end - c.a_start, ob = c.b_end - c.b_start;
    if (oa < p.min_overlap || ob < p.min_overlap) return KMU_SG_SHORT;
    if (aln) {
        const uint64_t m = aln->matches, e = aln->edit;
        if (!(aln->flags & KMU_ALN_DONE) || m * 1000ull < (uint64_t) p.min_identity_permille * (m + e)) return KMU_SG_LOWID;
    }
    const SgHangs h = sg_hangs(c, la, lb);
    const uint64_t hang = (h.aL < h.bL ? h.aL : h.bL) + (h.aR < h.bR ? h.aR : h.bR);
    const uint64_t maplen = oa > ob ? oa : ob;
    if (hang > p.max_hang || hang * 1000ull > maplen * (uint64_t) p.int_permille) return KMU_SG_INTERNAL;
    const bool a_in = h.aL <= h.bL && h.aR <= h.bR, b_in = h.aL >= h.bL && h.aR >= h.bR;
    if (a_in && b_in) return la < lb ? KMU_SG_A_CONTAINED : KMU_SG_B_CONTAINED;
    if (a_in) return KMU_SG_A_CONTAINED;
    if (b_in) return KMU_SG_B_CONTAINED;
    return KMU_SG_DOVETAIL;
}

// the two arcs of a DOVETAIL record: x leaves a vertex of read_a, y a vertex of read_b; each is the other's mate
KMU_SG_HD void sg_arc_pair(const kmu_chain &c, uint64_t la, uint64_t lb, uint32_t rec, kmu_sg_arc &x, kmu_sg_arc &y) {
    const SgHangs h = sg_hangs(c, la, lb);
    const uint32_t a2 = 2u * c.read_a, b2 = 2u * c.read_b, s = c.strand;
    if (h.aL > h.bL) {
        x.from = a2;
        x.to = b2 + s;
        x.len = (uint32_t) (h.bR - h.aR);
        y.from = b2 + (s ^ 1u);
        y.to = a2 + 1u;
        y.len = (uint32_t) (h.aL - h.bL);
    } else {
        x.from = a2 + 1u;
        x.to = b2 + (s ^ 1u);
        x.len = (uint32_t) (h.bL - h.aL);
        y.from = b2 + s;
        y.to = a2;
        y.len = (uint32_t) (h.aR - h.bR);
    }
    x.ovl = c.a_end - c.a_start;
    y.ovl = c.b_end - c.b_start;
    x.rec = y.rec = rec;
    x.flags = y.flags = x.unique = y.unique = x.zero = y.zero = 0u;
}
KMU_SG_HD uint64_t sg_arc_key(const kmu_sg_arc &a) { return ((uint64_t) a.from << 32) | a.to; }

// the first of the n sorted arcs whose `from` is >= v (n if there is none): where out(v) begins, and out(v - 1) ends
KMU_SG_HD uint64_t sg_lower_from(const kmu_sg_arc *arcs, uint64_t n, uint64_t v) {
    uint64_t lo = 0, hi = n; // every arc below lo has from < v, every arc from hi on has from >= v
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (arcs[mid].from < v) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}
// the first arc of the slice [lo, hi) whose `to` is >= x (hi if there is none): where the run of arcs -> x begins
KMU_SG_HD uint64_t sg_run_begin(const kmu_sg_arc *arcs, uint64_t lo, uint64_t hi, uint32_t x) {
    while (lo < hi) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (arcs[mid].to < x) lo = mid + 1u;
        else hi = mid;
    }
    return lo;
}

// the largest len of the slice [lo, hi) and the first arc that has the smallest one: first(v) under (len, to, rec), because the
// slice is in (to, rec) order.  An empty slice gives 0 and hi.
KMU_SG_HD void sg_vertex_stats(const kmu_sg_arc *arcs, uint64_t lo, uint64_t hi, uint32_t &max_len, uint64_t &first) {
    max_len = 0u;
    first = hi;
    uint32_t min_len = 0xFFFFFFFFu;
    for (uint64_t i = lo; i < hi; i++) {
        const uint32_t len = arcs[i].len;
        if (len > max_len) max_len = len;
        if (first == hi || len < min_len) {
            min_len = len;
            first = i;
        }
    }
}

// does the pair f = v -> w, g = w -> x eliminate the arcs v -> x
KMU_SG_HD bool sg_rule(uint32_t len_f, uint32_t len_g, uint32_t max_len_v, uint32_t fuzz, bool g_is_first) {
    return (uint64_t) len_f + len_g <= (uint64_t) max_len_v + fuzz || len_g < fuzz || g_is_first;
}

// one lane's step of the reduction: arc g = arcs[j] of out(w) against f = v -> w.  [v_lo, v_hi) is out(v), first_w the index of
// first(w).  Where the rule holds, mark(rec) is called for every arc of the run v -> x.
template <class Mark>
KMU_SG_HD void sg_reduce_step(const kmu_sg_arc *arcs, uint32_t len_f, uint64_t v_lo, uint64_t v_hi, uint32_t max_len_v, uint64_t j,
                              uint64_t first_w, uint32_t fuzz, Mark mark) {
    const uint32_t x = arcs[j].to;
    if (!sg_rule(len_f, arcs[j].len, max_len_v, fuzz, j == first_w)) return;
    for (uint64_t k = sg_run_begin(arcs, v_lo, v_hi, x); k < v_hi && arcs[k].to == x; k++) mark(arcs[k].rec);
}

} // namespace kmu

// kmu_ut_core.h -- the arithmetic of the unitig layout: which unique arcs the device may use as links, the mate test, the state of a
// vertex under pointer doubling and one round of it, the cut of a cycle, what a tail publishes, the step and the place of a vertex,
// the checks of a step list and the source byte of an output byte; for the device and for a host compiler alike
// (tests/cpp/sim_unitigs.cpp drives these functions over simulated lanes; the contract is in include/kmu.h).  The item that holds an
// output byte and the tile walk of the sequence copy are in kmu_gather_core.h.
//
// Doubling runs BACKWARDS over prev.  The state of v describes a SEGMENT: v, prev(v), ... up to but excluding anc; cnt vertices, dist
// the sum of their contributions, minv the smallest of them, top the last one.  A round joins the segment of v with that of anc.  On
// a path anc ends as KMU_SG_NONE: then cnt is rank + 1, dist the step's end, top the head.  On a cycle anc never does; cnt and dist
// count vertices twice (unsigned wrap is harmless, the cycle is cut and ranked again) and minv, being idempotent, is the cycle's
// smallest vertex once the segment has gone round.
#pragma once

#include <stdint.h>

#include "../../include/kmu.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_UT_HD __host__ __device__ __forceinline__
#else
#define KMU_UT_HD inline
#endif

namespace kmu {

static_assert(sizeof(kmu_sg_step) == 16 && sizeof(kmu_sg_unitig) == 32 && sizeof(kmu_sg_place) == 16, "the records of include/kmu.h");

// the doubling rounds that rank every path of up to n_v vertices: ceil(log2(n_v)), at least 1
KMU_UT_HD uint32_t ut_rounds(uint64_t n_v) {
    uint32_t r = 1;
    while ((1ull << r) < n_v) r++;
    return r;
}

// what can be said of a unique arc before any length or flag of a read is fetched
KMU_UT_HD bool ut_arc_range_ok(const kmu_sg_arc &a, uint32_t n_reads) {
    const uint64_t n_v = 2ull * n_reads;
    return a.from < n_v && a.to < n_v && (a.from >> 1) != (a.to >> 1) && !(a.flags & KMU_SG_ARC_REDUCED);
}
// and with the length of the `to` read and the flags of both reads (0 without summaries)
KMU_UT_HD bool ut_arc_reads_ok(const kmu_sg_arc &a, uint64_t len_to, uint32_t flags_from, uint32_t flags_to) {
    return a.len <= len_to && !((flags_from | flags_to) & KMU_SG_READ_CONTAINED);
}
// the mate test of vertex v whose link is next[v] = w: w^1 must link to v^1
KMU_UT_HD bool ut_mate_ok(const uint32_t *next, uint32_t v) {
    const uint32_t w = next[v];
    return w == KMU_SG_NONE || next[w ^ 1u] == (v ^ 1u);
}

struct UtState {
    uint32_t anc, cnt, top, minv;
};
// the contribution of v: the length of its in-arc if it has one (the start of a cut cycle keeps its), else that of its read
KMU_UT_HD uint64_t ut_contribution(uint32_t has_in, uint32_t in_len, uint64_t read_len) { return has_in ? (uint64_t) in_len : read_len; }
KMU_UT_HD UtState ut_state_init(uint32_t v, uint32_t prev) { return UtState{prev, 1u, v, v}; }
// one round for v: reads the states of the round before (s_in, d_in), returns v's next state
KMU_UT_HD UtState ut_round(const UtState *s_in, const uint64_t *d_in, uint32_t v, uint64_t &dist) {
    UtState s = s_in[v];
    dist = d_in[v];
    if (s.anc != KMU_SG_NONE) {
        const UtState a = s_in[s.anc];
        dist += d_in[s.anc];
        s.cnt += a.cnt;
        s.top = a.top;
        s.minv = a.minv < s.minv ? a.minv : s.minv;
        s.anc = a.anc;
    }
    return s;
}
// after the rounds: v lies on a cycle iff its segment never reached a head, and starts it iff it is the smallest vertex of it
KMU_UT_HD bool ut_cycle_start(const UtState &s, uint32_t v) { return s.anc != KMU_SG_NONE && s.minv == v; }
// of a path and its twin the one whose smallest vertex is even is kept
KMU_UT_HD bool ut_kept(uint32_t path_min) { return !(path_min & 1u); }

// ---- sequences ------------------------------------------------------------------------------------------------------------------
// a unitig's slice of the step list
KMU_UT_HD bool ut_slice_ok(const kmu_sg_unitig &u, uint64_t n_steps) {
    return u.first <= n_steps && u.n_reads <= n_steps - u.first && (u.n_reads || u.len == 0);
}
// one step of a unitig: prev_end is 0 at the first step; read_len is only valid if s.read < n_reads (the caller passes 0 otherwise)
KMU_UT_HD bool ut_step_ok(const kmu_sg_step &s, uint32_t n_reads, uint64_t prev_end, uint64_t read_len, bool last, uint64_t len) {
    return s.read < n_reads && s.strand <= 1u && s.end >= prev_end && s.end - prev_end <= read_len && (!last || s.end == len);
}
KMU_UT_HD uint8_t ut_complement(uint8_t b) {
    switch (b) {
    case 'A': return 'T';
    case 'C': return 'G';
    case 'G': return 'C';
    case 'T': return 'A';
    case 'a': return 't';
    case 'c': return 'g';
    case 'g': return 'c';
    case 't': return 'a';
    default: return 'N';
    }
}
// byte k of a step's c bytes (the last c of the read in the step's orientation) as an index into the read of length read_len
KMU_UT_HD uint64_t ut_src_index(uint32_t strand, uint64_t read_len, uint64_t c, uint64_t k) { return strand ? c - 1u - k : read_len - c + k; }

} // namespace kmu

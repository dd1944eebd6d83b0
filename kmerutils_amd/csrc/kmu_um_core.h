// kmu_um_core.h -- the arithmetic of the unitig map: the checks of a unitig, a step, a place and a containment record, the record of
// a layout read, the candidate a containment record makes, its projection through the container's place, the key of the atomic
// maximum and the record of the winner; for the device and for a host compiler alike (tests/cpp/sim_unitig_map.cpp drives these
// functions over simulated lanes; the contract is in include/kmu.h).
#pragma once

#include <stdint.h>

#include "../../include/kmu.h"

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_UM_HD __host__ __device__ __forceinline__
#else
#define KMU_UM_HD inline
#endif

namespace kmu {

static_assert(sizeof(kmu_um_params) == 8 && sizeof(kmu_um_stats) == 24 && sizeof(kmu_chain) == 40, "the records of include/kmu.h");

// ---- checks -------------------------------------------------------------------------------------------------------------------------
KMU_UM_HD bool um_unitig_ok(const kmu_sg_unitig &u, uint64_t n_steps) {
    return u.first <= n_steps && u.n_reads <= n_steps - u.first && u.len < 0x100000000ull;
}
KMU_UM_HD bool um_step_ok(const kmu_sg_step &s, uint32_t n_reads) { return s.read < n_reads && s.strand <= 1u && s.end != 0ull; }
// the place of read r; every record it names is checked before it is used as an index, so the order of the checks does not matter
KMU_UM_HD bool um_place_ok(const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path, uint64_t n_steps,
                           const kmu_sg_place &p, uint32_t r) {
    if (p.unitig == KMU_SG_NONE) return true;
    if (p.unitig >= n_unitigs) return false;
    const kmu_sg_unitig u = unitigs[p.unitig];
    if (!um_unitig_ok(u, n_steps) || p.rank >= u.n_reads) return false;
    const kmu_sg_step s = path[u.first + p.rank];
    return s.read == r && s.strand == p.strand && s.strand <= 1u && s.end != 0ull && s.end <= u.len;
}
KMU_UM_HD bool um_is_containment(uint32_t cls) { return cls == KMU_SG_A_CONTAINED || cls == KMU_SG_B_CONTAINED; }
// a containment record before it is used as an index: the reads exist (then, and only then, the caller passes their lengths)
KMU_UM_HD bool um_rec_reads_ok(const kmu_chain &x, uint32_t n_reads) { return x.read_a < n_reads && x.read_b < n_reads && x.strand <= 1u; }
KMU_UM_HD bool um_rec_segs_ok(const kmu_chain &x, uint64_t len_a, uint64_t len_b) {
    return x.a_start <= x.a_end && x.a_end <= len_a && x.b_start <= x.b_end && x.b_end <= len_b;
}

// ---- layout reads ---------------------------------------------------------------------------------------------------------------
// read r of length L with the place {u, rank, s} whose step ends at e (the place has passed um_place_ok: 0 < e < 2^32)
KMU_UM_HD kmu_chain um_layout_record(uint32_t u, uint32_t r, uint32_t s, uint64_t e, uint64_t L) {
    const uint64_t t = L < e ? L : e;
    kmu_chain c;
    c.read_a = u;
    c.read_b = r;
    c.strand = s;
    c.score = 0u;
    c.n_seeds = KMU_SG_NONE;
    c.n_anchors = KMU_SG_NONE;
    c.a_start = (uint32_t) (e - t);
    c.a_end = (uint32_t) e;
    c.b_start = (uint32_t) (s ? 0ull : L - t);
    c.b_end = (uint32_t) (s ? t : L);
    return c;
}

// ---- contained reads ------------------------------------------------------------------------------------------------------------
struct UmCand {
    uint32_t c, g;           // the contained read and its container
    uint32_t cs, ce, gs, ge; // their segments
};
// the candidate a record of class A_CONTAINED or B_CONTAINED makes
KMU_UM_HD UmCand um_cand(const kmu_chain &x, uint32_t cls) {
    if (cls == KMU_SG_A_CONTAINED) return UmCand{x.read_a, x.read_b, x.a_start, x.a_end, x.b_start, x.b_end};
    return UmCand{x.read_b, x.read_a, x.b_start, x.b_end, x.a_start, x.a_end};
}
// where g's segment begins on g's unitig: g's step is (sg, e_g), its length L_g; below 0 the candidate is dropped
KMU_UM_HD int64_t um_project(const UmCand &k, uint32_t sg, uint64_t e_g, uint64_t L_g) {
    const int64_t os = sg ? (int64_t) L_g - (int64_t) k.ge : (int64_t) k.gs;
    return (int64_t) e_g - (int64_t) L_g + os;
}
// the key of the atomic maximum: the longest segment of c wins, then the smallest record index x (< 2^32 - 1, so a key is never 0)
KMU_UM_HD unsigned long long um_key(const UmCand &k, uint64_t x) {
    return ((unsigned long long) (k.ce - k.cs) << 32) | (unsigned long long) (0xFFFFFFFFu - (uint32_t) x);
}
KMU_UM_HD uint32_t um_key_index(unsigned long long key) { return 0xFFFFFFFFu - (uint32_t) (key & 0xFFFFFFFFull); }
// the record of the winner x: u_g and sg of g's place, a_start = um_project(...) >= 0
KMU_UM_HD kmu_chain um_contained_record(const UmCand &k, uint32_t x, uint32_t x_strand, uint32_t u_g, uint32_t sg, int64_t a_start) {
    kmu_chain c;
    c.read_a = u_g;
    c.read_b = k.c;
    c.strand = sg ^ x_strand;
    c.score = 1u;
    c.n_seeds = x;
    c.n_anchors = k.g;
    c.a_start = (uint32_t) a_start;
    c.a_end = (uint32_t) (a_start + (int64_t) (k.ge - k.gs));
    c.b_start = k.cs;
    c.b_end = k.ce;
    return c;
}

} // namespace kmu

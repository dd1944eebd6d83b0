// kmu_count_plan.hpp -- the host arithmetic of the partitioned build (kmu_count_part.hip): numbers in, numbers out, no HIP
// header, so that the host-only sanitizer program (tests/cpp/test_host_san.cpp) compiles it with g++ alone.
#pragma once

#include <stdint.h>

#include <algorithm>
#include <cmath>

namespace kmu {

// wave steps of a flat stream of `bases` bases: a lane takes a 16-base word, a wave 64 of them.  constexpr: the kernels call it
// too (hipcc compiles a constexpr function for host and device alike), g++ sees plain C++.
constexpr uint64_t flat_wave_steps(uint64_t bases) { return ((bases + 15) / 16 + 63) / 64; }

// The wave steps of a stream dealt out to at most `unit_cap` units (workgroups) of steps_per_unit consecutive steps each; no
// steps at all: one unit of one step.  asked: the unit count before it is re-rounded to what steps_per_unit leaves (the
// censuses derive their sample shift from it).
struct UnitSplit { uint32_t units, steps_per_unit; uint64_t asked; };
inline UnitSplit unit_split(uint64_t nsteps, uint64_t unit_cap) {
    const uint64_t n = std::max<uint64_t>(nsteps, 1);
    UnitSplit s;
    s.asked = std::min(n, unit_cap);
    s.steps_per_unit = (uint32_t) ((n + s.asked - 1) / s.asked);
    s.units = (uint32_t) ((n + s.steps_per_unit - 1) / s.steps_per_unit);
    return s;
}

// ---- the single-pass partition: capacity of a stream that expects `mean` items; share: 1, or KMU_COUNT_SEG_PCT / 100 (tests: force overflows)
inline uint64_t seg_cap_for(double mean, double share) {
    // 5 sigma of independent k-mers: three streams in ten million overflow, by a few items that the spill list takes
    const double cap = (mean + 5.0 * std::sqrt(mean) + 32.0) * share;
    // whole 128-byte lines, never below the bound (rounded up before the lines: it used to be cut to a whole number first, which
    // left a stream a fraction of an item short of it where that number was a multiple of 16)
    return ((uint64_t) std::ceil(cap) + 15) & ~(uint64_t) 15;
}
// level 1: sets of shared streams, two per XCD (bench workload, same box: 15.8-16.1 ms; one per XCD 18.5, four 15.9-16.7, eight
// 20.3, one for the whole chip 19.8-20.1, a unit's own streams 17.6-21.5 in two states).  Level 2: units per level-1 bin that
// share the bin's leaves (one unit with its own leaves: 23.5-24.2 ms; shared by 1 / 2 / 4 / 8 / 16 / 32 / 64 / 128 units: 21.6 /
// 22.3 / 20.3-21.4 / 18.5 / 16.9-17.4 / 17.7-17.9 / 17.9 / 20.0)
static constexpr uint32_t SEG_SETS = 16, SEG_L2_UNITS = 16;
struct SegPlan {
    uint32_t units1, steps_per_unit, sets;
    uint64_t cap1, cap2; // items per level-1 stream (set, bin) / per leaf
};
// over the reads of a flat stream into bins1 groups of n2 regions
inline SegPlan seg_plan(uint32_t num_cus, uint64_t total_bases, uint32_t bins1, uint32_t n2, double share) {
    // units of level 1: one workgroup per CU; under the upload of kmu_sketch_count the same units take a slice of every arrival
    const UnitSplit us = unit_split(flat_wave_steps(total_bases), num_cus);
    SegPlan sp{us.units, us.steps_per_unit, std::min(SEG_SETS, us.units), 0, 0};
    const uint64_t units_per_set = (sp.units1 + sp.sets - 1) / sp.sets;
    sp.cap1 = seg_cap_for((double) units_per_set * sp.steps_per_unit * 1024.0 / bins1, share);
    sp.cap2 = seg_cap_for((double) total_bases / bins1 / n2, share);
    return sp;
}
// over an array of n items: level 1 cuts it into one unit per CU (the biggest streams, the smallest margins)
inline SegPlan seg_plan_array(uint32_t num_cus, uint64_t n, uint32_t bins1, uint32_t n2, double share) {
    SegPlan sp{num_cus, 0, std::min(SEG_SETS, num_cus), 0, 0};
    sp.cap1 = seg_cap_for((double) n / sp.sets / bins1, share);
    sp.cap2 = seg_cap_for((double) n / bins1 / n2, share);
    return sp;
}

// One round of level 1 under an upload: the wave steps (1 024 bases each) that with their 32-base halo lie inside the first
// `bases_ready` bases and have not been through level 1 (steps_done).  An arrival of fewer than min_per_unit steps per unit
// waits for the next one; the last round (bases_ready >= total_bases) takes whatever is left.
struct SegRound {
    bool launch;    // n_new != 0: steps [steps_done, steps_done + n_new) go through level 1 now (a round that waits: 0)
    uint64_t n_new;
    bool last;      // every step has been through level 1 after this round
};
inline SegRound seg_round(uint64_t total_bases, uint64_t bases_ready, uint64_t steps_done, uint32_t units1, uint64_t min_per_unit) {
    const bool last = bases_ready >= total_bases;
    const uint64_t steps_ready = last ? flat_wave_steps(total_bases) : (bases_ready >= 32 ? (bases_ready - 32) / 1024 : 0);
    const uint64_t n_new = steps_ready > steps_done ? steps_ready - steps_done : 0;
    if (!last && n_new < (uint64_t) units1 * min_per_unit) return SegRound{false, 0, false};
    return SegRound{n_new != 0, n_new, last};
}

// the exact levels: 2^region_bits leaves (<= 22 bits) as 2^b1 groups of n2: one level up to 11 bits (b1 = 0), else two of about half the bits each
inline void region_split(int region_bits, int *b1, uint32_t *n2) {
    *b1 = region_bits <= 11 ? 0 : (region_bits + 1) / 2;
    *n2 = 1u << (region_bits - *b1);
}

} // namespace kmu

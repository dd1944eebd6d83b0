// kmu_kfilter_core.h -- the arithmetic of the count prefilter (kmu_kfilter, include/kmu.h), for the device and for a host compiler
// alike: the hash, the cell and the mask of a key, the class of a key from its cell, and the two host formulas (the size of a
// filter, the cardinality estimate).  No HIP call: a host-only program can include it (the numpy model of tests/kfilter_model.py
// restates the same lines).
//
// A filter is n_cells cells of 16 bytes {uint64 A, uint64 B}.  A key v sets up to n_hashes bits (its mask) of ONE cell.  Plane A:
// the OR of the masks that landed in the cell.  Plane B: bit b = "at least two occurrences landed on bit b".
#pragma once

#include <math.h>
#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_KF_HD __host__ __device__ __forceinline__
#else
#define KMU_KF_HD inline
#endif

namespace kmu {

constexpr uint32_t KF_MAX_HASHES = 8;
constexpr uint64_t KF_MAX_CELLS = 0xFFFFFFFFull; // cell = mulhi32(h >> 32, n_cells)

// splitmix64's finaliser over the next state
KMU_KF_HD uint64_t kf_sm(uint64_t z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// where key v lives and which bits it sets; coinciding positions collapse
KMU_KF_HD void kf_cell_mask(uint64_t v, uint64_t n_cells, uint32_t n_hashes, uint64_t &cell, uint64_t &mask) {
    const uint64_t h = kf_sm(v);
    uint64_t g = kf_sm(h);
    cell = ((h >> 32) * n_cells) >> 32;
    mask = 0;
    for (uint32_t i = 0; i < n_hashes; i++, g >>= 6) mask |= 1ull << (g & 63u);
}

// 0: never added; 1: added exactly once; 2: may have been added twice or more
KMU_KF_HD uint32_t kf_class(uint64_t a, uint64_t b, uint64_t mask) { return (a & mask) != mask ? 0u : ((b & mask) != mask ? 1u : 2u); }

// max(1, ceil(expected_distinct * bits_per_kmer / 64)) cells; 0 when that exceeds 2^32 - 1
inline uint64_t kf_cells_for(uint64_t expected_distinct, uint32_t bits_per_kmer) {
    if (expected_distinct == 0 || bits_per_kmer == 0) return 1;
    if (expected_distinct > (0xFFFFFFFFFFFFFFFFull - 63u) / bits_per_kmer) return 0; // the product alone is past 2^64
    const uint64_t cells = (expected_distinct * bits_per_kmer + 63u) / 64u;
    return cells > KF_MAX_CELLS ? 0 : cells;
}

// -(m / n_hashes) ln(1 - X / m), m = 64 n_cells bits of plane A of which X are set; INFINITY when the plane is full
inline double kf_est_distinct(uint64_t n_cells, uint32_t n_hashes, uint64_t bits_a) {
    const double m = 64.0 * (double) n_cells;
    if ((double) bits_a >= m) return INFINITY;
    return -(m / (double) n_hashes) * log(1.0 - (double) bits_a / m);
}

} // namespace kmu

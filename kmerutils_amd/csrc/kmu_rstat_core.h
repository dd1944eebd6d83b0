// kmu_rstat_core.h -- the arithmetic of the read statistics (kmu_read_stats, kmu_read_qual_stats, kmu_quality_remap; include/kmu.h),
// for the device and for a host compiler alike: the class of a base and of a quality byte, the rounded percentage, the bucket of a
// length in HdrHistogram's layout with its range, and the layout of a histogram.  Integers only, no HIP call: a host-only program
// can include it (tests/cpp/rstat_core_check.cpp; the numpy model of tests/read_stats_model.py restates the same lines).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_RS_HD __host__ __device__ __forceinline__
#else
#define KMU_RS_HD inline
#endif

namespace kmu {

constexpr uint32_t RS_BASE_CLASSES = 5; // A C G T other
constexpr uint32_t RS_QUAL_CLASSES = 8; // remap_quality8, src/quality/quality.rs:33-43
constexpr uint32_t RS_PCT_ROWS = 101;   // percentages 0 .. 100
constexpr uint32_t RS_NO_BUCKET = 0xFFFFFFFFu;

// A/a 0, C/c 1, G/g 2, T/t 3, every other byte 4 (Sequence::base_count, src/base/sequence.rs:333-364, on either case)
KMU_RS_HD uint32_t rs_base_class(uint32_t byte) {
    const uint32_t u = byte & 0xDFu;
    return u == 'A' ? 0u : u == 'C' ? 1u : u == 'G' ? 2u : u == 'T' ? 3u : 4u;
}

// remap_quality8: 0 below 0x25, then one class per three values, 7 from 0x37 on
KMU_RS_HD uint32_t rs_qual_class(uint32_t q) {
    if (q < 0x25u) return 0u;
    const uint32_t c = 1u + (q - 0x25u) / 3u;
    return c < 7u ? c : 7u;
}

// ((100 h) as f64 / L as f64).round() of statutils.rs:255-256 in integers: ties go up, 0 for an empty read.  h <= len < 2^55.
KMU_RS_HD uint32_t rs_pct(uint64_t h, uint64_t len) { return len ? (uint32_t) ((200u * h + len) / (2u * len)) : 0u; }

// ceil(log2(2 * 10^sig_digits)) for sig_digits 1 .. 5; 0 otherwise
KMU_RS_HD uint32_t rs_sub_bits(int sig_digits) {
    return sig_digits == 1 ? 5u : sig_digits == 2 ? 8u : sig_digits == 3 ? 11u : sig_digits == 4 ? 15u : sig_digits == 5 ? 18u : 0u;
}

KMU_RS_HD uint32_t rs_floor_log2(uint64_t v) { // v > 0
    uint32_t l = 0;
    while (v >>= 1) l++;
    return l;
}

// the bucket of a length: one each below 2^sub_bits, then every power-of-two range cut into 2^(sub_bits - 1)
KMU_RS_HD uint64_t rs_len_bucket(uint64_t len, uint32_t sub_bits) {
    const uint32_t fl = len ? rs_floor_log2(len) : 0u;
    const uint32_t shift = fl > sub_bits - 1u ? fl - (sub_bits - 1u) : 0u;
    return ((uint64_t) shift << (sub_bits - 1u)) + (len >> shift);
}

// the lowest and the highest length of a bucket
KMU_RS_HD void rs_bucket_range(uint64_t bucket, uint32_t sub_bits, uint64_t &lowest, uint64_t &highest) {
    const uint64_t q = bucket >> (sub_bits - 1u);
    const uint64_t shift = q > 1u ? q - 1u : 0u;
    lowest = shift < 64u ? (bucket - (shift << (sub_bits - 1u))) << shift : 0u;
    highest = lowest + ((shift < 64u ? (uint64_t) 1 << shift : 0u) - 1u);
}

// Histogram::new_with_bounds(1, max_len, sig_digits): the number of buckets and the first length that has none
KMU_RS_HD void rs_len_layout(uint64_t max_len, uint32_t sub_bits, uint32_t &n_buckets, uint64_t &limit) {
    uint32_t ranges = 1; // the smallest j >= 1 with 2^sub_bits * 2^(j - 1) > max_len
    while (sub_bits + ranges - 1u < 64u && ((uint64_t) 1 << (sub_bits + ranges - 1u)) <= max_len) ranges++;
    limit = sub_bits + ranges - 1u < 64u ? (uint64_t) 1 << (sub_bits + ranges - 1u) : ~(uint64_t) 0; // (2^64 does not fit)
    n_buckets = (ranges + 1u) << (sub_bits - 1u);
}

// the smallest class c with 2 * (n[0] + .. + n[c]) >= len; 0 for an empty read
KMU_RS_HD uint32_t rs_median_class(const uint64_t *n, uint64_t len) {
    uint64_t run = 0;
    for (uint32_t c = 0; c < RS_QUAL_CLASSES; c++) {
        run += n[c];
        if (2u * run >= len) return c;
    }
    return RS_QUAL_CLASSES - 1u;
}

} // namespace kmu

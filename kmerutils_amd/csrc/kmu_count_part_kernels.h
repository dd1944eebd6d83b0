// kmu_count_part_kernels.h -- what the host side of the partitioned build (kmu_count_part.hip: routes, buffers, launches) needs of
// its kernels (one file per stage: kmu_count_part_level1.hip, kmu_count_part_array.hip, kmu_count_part_build.hip): their plan blocks,
// the constants and byte functions their launches and LDS budgets are made of, and their declarations (every kernel file instantiates
// the template kernels it defines for exactly the forms listed here).
#pragma once

#include "kmu_count_table.h"

namespace kmu {

// the LDS-staged scatters: a 1024-thread workgroup sorts a tile of <= 16384 items
static constexpr uint32_t TILE_ITEMS = 16384;
static constexpr int SCATTER_THREADS = 1024;
static size_t scatter_lds_bytes(uint32_t nbins) { return (size_t) TILE_ITEMS * 8 + (size_t) nbins * 8 + ((size_t) nbins + 1 + 16) * 4 + 16; }
static size_t seg_lds_bytes(uint32_t nbins, bool lox = false) { return (size_t) TILE_ITEMS * 8 + ((size_t) nbins * 3 + 4) * 4 + 64 + (lox ? (size_t) nbins * 4 : 0); }
static constexpr uint32_t LEAF6_MAX_BINS = 2024; // (with the lox copy the tile sort of 2 048 bins would need 80 bytes more than a CU's 160 KiB)

// What a partition item is: IT_HASH = khash(key) (digit = a function of the item), IT_KEY = the key itself (digit from
// khash(key)), IT_OWNER = the key, digit = its owner in a key partition (DispatchableT, kmercount.rs:382-420; the Digit then
// carries kmer_owner's mode in `sh` and the number of parts in `n2`), IT_KEY_TO_HASH: keys in, khash(key) out.
enum { IT_HASH = 0, IT_KEY = 1, IT_OWNER = 2, IT_KEY_TO_HASH = 3 };

// the rounds of k_part_scatter1 (level 1 of the single-pass partition)
struct SegPlan1 {
    uint64_t cap, step_base, step_end;
    uint32_t *ovf, *err, *state;
    uint32_t sets;
    const uint16_t *novalid; // flat_novalid's bits of all wave steps of the stream
};

// the generic radix partition of a u64 array: `nparts` consecutive input partitions (bounds[nparts + 1]), each cut into `chunks`
// units; a unit scatters its slice by the digit `d` into `bins` sub-partitions
struct ArrPlan {
    Digit d;
    uint32_t bins;
    uint32_t nparts;
    uint32_t chunks;
    // single-pass form: != 0: the input partition p is not contiguous but the p-th stream (seg_cap items) of each of seg_units
    // blocks of seg_bins streams -- what the single-pass level 1 leaves, one block per set; bounds is not read
    uint32_t seg_units, seg_cap, seg_bins;
    // single-pass form, level 1 of an array: > 1 = that many sets of shared output streams, a unit writes set blockIdx.x % out_sets
    // ([set][bin][cap], cursors in the same order); 0 / 1: one set per input partition (level 2: the leaves)
    uint32_t out_sets;
};

// the region build
static constexpr int BUILD_THREADS = 1 << (REGION_BITS_MAX - 3); // 512 threads for regions of 4096 slots
static constexpr int BUILD_PRE = 6;
// batched form of the quotient build: entries of the per-wave pool of items that two probes did not place (8 bytes each, behind the
// region in LDS: 32 + 6 KiB per workgroup, four workgroups per CU as before)
static constexpr uint32_t BUILD_POOL = 96, BUILD_PASSES = 3; // batched probes of an item before it goes to the pool (1 / 2 / 3: 21.1 / 18.8 / 18.4 ms)

// ---- the kernels (definitions and comments: kmu_count_part_level1.hip, kmu_count_part_array.hip, kmu_count_part_build.hip) -----------
// (every declaration carries the launch bounds of its definition: the `extern template` lines below instantiate the declaration they
//  see, and a bound that only the definition has is then lost -- k_part_build_q's four workgroups per CU rest on its bound)
// kmu_count_part_level1.hip
__global__ void __launch_bounds__(256) k_part_hist1(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, PartPlan pl, uint32_t *hist1,
                                                    uint32_t *err, SampleArgs sa);
__global__ void __launch_bounds__(256) k_sample_distinct(const uint64_t *list, uint32_t n, uint64_t *table, uint32_t mask, uint32_t *n_distinct);
__global__ void __launch_bounds__(256) k_part_scan1a(const uint32_t *hist1, PartPlan pl, uint64_t *offs1, uint64_t *tot1);
__global__ void __launch_bounds__(256) k_part_scan1b(const uint64_t *tot1, PartPlan pl, uint64_t *binstart1);
__global__ void __launch_bounds__(SCATTER_THREADS) k_part_scatter1_exact(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, PartPlan pl,
                                                                         const uint64_t *offs1, const uint64_t *binstart1, uint64_t *out);
__global__ void __launch_bounds__(SCATTER_THREADS) k_part_scatter1(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, PartPlan pl,
                                                                   uint64_t *out, SegPlan1 seg);
// kmu_count_part_array.hip
template <int IT>
__global__ void __launch_bounds__(256) k_arr_hist(const uint64_t *in, const uint64_t *bounds, ArrPlan pl, uint32_t *hist);
__global__ void __launch_bounds__(256) k_arr_scan_a(const uint32_t *hist, ArrPlan pl, uint32_t T, uint64_t *offs_rel, uint64_t *tot);
__global__ void __launch_bounds__(256) k_arr_scan_b(const uint64_t *tot, const uint64_t *bounds, ArrPlan pl, uint64_t *outbounds);
template <int IT>
__global__ void __launch_bounds__(SCATTER_THREADS) k_arr_scatter_exact(const uint64_t *in, const uint64_t *bounds, ArrPlan pl, const uint64_t *offs_rel,
                                                                       const uint64_t *outbounds, uint64_t *out);
template <int IT, bool LEAF6>
__global__ void __launch_bounds__(SCATTER_THREADS) k_arr_scatter_seg(const uint64_t *in, const uint64_t *bounds, ArrPlan pl, uint64_t *out, uint64_t seg_cap,
                                                                     uint32_t *seg_ovf, uint32_t *leafcnt, const uint32_t *lox);
__global__ void __launch_bounds__(SCATTER_THREADS) k_smer_scatter1(const uint32_t *recs, uint64_t n_rec, int k, ArrPlan pl, uint64_t *out, uint64_t seg_cap,
                                                                   uint32_t *seg_ovf, uint32_t *cursors);
__global__ void __launch_bounds__(64) k_spill_header(uint32_t *ovf, uint32_t cap, uint64_t *list);
__global__ void __launch_bounds__(256) k_seg_tails(const uint32_t *cursor, uint32_t n_streams, uint32_t cap, uint64_t *out);
__global__ void __launch_bounds__(256) k_fill_linear(uint64_t *out, uint64_t n, uint64_t stride);
// kmu_count_part_build.hip
template <int IT, bool LEAF6>
__global__ void __launch_bounds__(BUILD_THREADS, 8) k_part_build_q(const uint64_t *__restrict__ items, const uint64_t *__restrict__ leafstart,
                                                                   uint32_t n_regions, CountTable t, int in_mode, uint32_t *err, uint64_t leaf_stride,
                                                                   const uint32_t *__restrict__ leafcnt);
template <int IT>
__global__ void __launch_bounds__(BUILD_THREADS) k_part_build(const uint64_t *__restrict__ items, const uint64_t *__restrict__ leafstart, uint32_t n_regions,
                                                              CountTable t, int in_mode, uint32_t *err, uint64_t leaf_stride,
                                                              const uint32_t *__restrict__ leafcnt);
__global__ void __launch_bounds__(256) k_count_add_spill(const uint64_t *items, const uint32_t *ovf, CountTable t, uint32_t *err);

// the forms of the template kernels the host launches, by the file that defines and instantiates them; declared for everybody
#define KMU_COUNT_PART_ARRAY_FORMS(X)                                                                                                \
    X(k_arr_hist<IT_HASH>(const uint64_t *, const uint64_t *, ArrPlan, uint32_t *))                                                  \
    X(k_arr_hist<IT_KEY>(const uint64_t *, const uint64_t *, ArrPlan, uint32_t *))                                                   \
    X(k_arr_scatter_exact<IT_HASH>(const uint64_t *, const uint64_t *, ArrPlan, const uint64_t *, const uint64_t *, uint64_t *))         \
    X(k_arr_scatter_exact<IT_KEY>(const uint64_t *, const uint64_t *, ArrPlan, const uint64_t *, const uint64_t *, uint64_t *))          \
    X(k_arr_scatter_exact<IT_KEY_TO_HASH>(const uint64_t *, const uint64_t *, ArrPlan, const uint64_t *, const uint64_t *, uint64_t *))  \
    X(k_arr_scatter_seg<IT_HASH, false>(const uint64_t *, const uint64_t *, ArrPlan, uint64_t *, uint64_t, uint32_t *, uint32_t *, const uint32_t *))        \
    X(k_arr_scatter_seg<IT_HASH, true>(const uint64_t *, const uint64_t *, ArrPlan, uint64_t *, uint64_t, uint32_t *, uint32_t *, const uint32_t *))         \
    X(k_arr_scatter_seg<IT_KEY_TO_HASH, false>(const uint64_t *, const uint64_t *, ArrPlan, uint64_t *, uint64_t, uint32_t *, uint32_t *, const uint32_t *))
#define KMU_COUNT_PART_BUILD_FORMS(X)                                                                                                \
    X(k_part_build_q<IT_HASH, false>(const uint64_t *__restrict__, const uint64_t *__restrict__, uint32_t, CountTable, int, uint32_t *, uint64_t, const uint32_t *__restrict__)) \
    X(k_part_build_q<IT_HASH, true>(const uint64_t *__restrict__, const uint64_t *__restrict__, uint32_t, CountTable, int, uint32_t *, uint64_t, const uint32_t *__restrict__))  \
    X(k_part_build_q<IT_KEY, false>(const uint64_t *__restrict__, const uint64_t *__restrict__, uint32_t, CountTable, int, uint32_t *, uint64_t, const uint32_t *__restrict__))  \
    X(k_part_build<IT_HASH>(const uint64_t *__restrict__, const uint64_t *__restrict__, uint32_t, CountTable, int, uint32_t *, uint64_t, const uint32_t *__restrict__))           \
    X(k_part_build<IT_KEY>(const uint64_t *__restrict__, const uint64_t *__restrict__, uint32_t, CountTable, int, uint32_t *, uint64_t, const uint32_t *__restrict__))
#define KMU_COUNT_PART_KERNEL_FORMS(X) KMU_COUNT_PART_ARRAY_FORMS(X) KMU_COUNT_PART_BUILD_FORMS(X)
#define KMU_X_EXTERN(...) extern template __global__ void __VA_ARGS__;
KMU_COUNT_PART_KERNEL_FORMS(KMU_X_EXTERN)
#undef KMU_X_EXTERN

} // namespace kmu

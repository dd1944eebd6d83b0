// kmu_sketch_host.hpp -- the host side of the sketch unit: what its .hip files call in each other, and the small rules that more
// than one of them (host or device code) states.  kmu_sketch.hip: entry points, the all-sequences path, the shared helpers;
// kmu_sketch_pmh.hip: ProbMinHash3a / bottom-k routes; kmu_sketch_pipe.hip: kmu_sketch_count; kmu_sketch_super.hip,
// kmu_sketch_dens.hip, kmu_sketch_groups.hip: kernels and launchers of their own (what the last two share: kmu_sketch_dens.h).
#pragma once

#include <algorithm>

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

// ---- rules ----
// bytes per signature element
inline size_t sig_elem_bytes(int sig_type) {
    return sig_type == KMU_SIG_U16 ? 2 : (sig_type == KMU_SIG_U32 || sig_type == KMU_SIG_F32) ? 4 : 8;
}
// the sketches kept as m bins / registers with one independent update per k-mer occurrence (kmu_sketch_dens.hip)
inline bool algo_is_dens(int algo) { return algo == KMU_ALGO_OPTDENS || algo == KMU_ALGO_REVOPTDENS || algo == KMU_ALGO_HLL; }
// SuperMinHash signature form: 0 f64, 1 f32, 2 u64 (SuperMinHash2), 3 u32 (SuperMinHash2)
inline int super_mode(const kmu_sketch_params *p) {
    return p->algo == KMU_ALGO_SUPER ? (p->sig_type == KMU_SIG_F32 ? 1 : 0) : (p->sig_type == KMU_SIG_U32 ? 3 : 2);
}
// the initial slot pattern of a SuperMinHash form: F::from(u32::MAX) as f64 (4294967295.0) / f32 (4294967296.0f), all ones of u64 / u32
__host__ __device__ inline uint64_t super_init_bits(int mode) {
    switch (mode) {
    case 0: return 0x41EFFFFFFFE00000ull;
    case 1: return 0x4F800000ull;
    case 2: return 0xFFFFFFFFFFFFFFFFull;
    default: return 0xFFFFFFFFull;
    }
}
// ProbMinHash3a over n pre-hashed values: 2^bits leaves of ~4k keys, comfortably inside one LDS pass even with a skewed hash
__host__ __device__ inline uint32_t pmh_leaf_bits(uint64_t n) {
    uint32_t b = 0;
    while (b < 22 && (n >> b) > 4096) b++;
    return b;
}
// k_multiset_long: a read of nk k-mers is cut into ceil(nk / PMH_LONG_TP) sub-lists by key hash.  At 16 384 keys a sub-list expects
// n^2 / 2^18 = 1 024 keys in collision groups (of UQ2_COLL = 2 048) and stays 4 096 keys (~ 30 standard deviations) under the 20 480 that
// a workgroup's registers hold.  The per-sequence route keeps reads of up to LONG_SEQ_KMERS = 2^18 k-mers: at most 16 sub-lists.
// (Measured on the ONT workload, the stage per step: 12 288: 3.19 - 3.22 ms, 14 336: 3.17 - 3.18, 16 384: 3.11 - 3.15)
static constexpr uint32_t PMH_LONG_TP = 16384;
__host__ __device__ inline uint32_t pmh_long_parts(uint32_t nk) { return nk / PMH_LONG_TP + (nk % PMH_LONG_TP ? 1u : 0u); }
// the sub-list of a key, 0 .. parts - 1.  The bitmap index and the collision sort's bucket of k_multiset_uq's step are both functions of
// lo ^ hi of the key; this is one of lo + c hi, so the keys of one sub-list still spread evenly over bitmap bits and buckets.
__host__ __device__ inline uint32_t pmh_long_part_of(uint64_t key, uint32_t parts) {
    const uint32_t z = ((uint32_t) key + (uint32_t) (key >> 32) * 0x9E3779B9u) * 0xC2B2AE3Du;
    return (uint32_t) (((uint64_t) z * parts) >> 32);
}
// SuperMinHash(2) over n pre-hashed values: chunks of at most 16 384, between 1 and 8192 of them
__host__ __device__ inline uint64_t super_chunk_count(uint64_t n) {
    const uint64_t c = (n + 16383) / 16384;
    return c < 1 ? 1 : (c > 8192 ? 8192 : c);
}
// The launch shape of k_sketch_super for a sketch of m slots that stages `chunk` items, on a device that gives a workgroup lds_max
// bytes of LDS.  The kernel carves 16 m + 8 chunk + 16 bytes (slot minima, staged seeds, index bounds, two words) and one
// permutation column of m entries per item lane out of `lds`; an entry is one byte up to m = 256 and two above (`wide`).  The
// columns dominate: the workgroup shrinks from 256 to 64 threads (every thread an item lane) until they fit, and beyond that one
// wave keeps as many item lanes as columns fit.  ncol == 0: not even one column fits, the launcher refuses the sketch size.
struct SuperPlan {
    int threads;       // workgroup size
    int ncol;          // item lanes that own a permutation column (<= threads)
    int wide;          // two-byte permutation entries
    size_t lds;        // dynamic LDS of the launch, a multiple of 16
    int blocks_per_cu; // workgroups per CU of the grid
};
inline SuperPlan super_plan(int m, uint32_t chunk, size_t lds_max) {
    SuperPlan sp;
    sp.wide = m > 256 ? 1 : 0;
    const size_t pt = sp.wide ? 2 : 1;
    sp.threads = 256;
    sp.lds = 0;
    sp.ncol = 0;
    for (; sp.threads >= 64; sp.threads -= 64) {
        sp.lds = (size_t) 16 * m + (size_t) 8 * chunk + 16 + pt * m * sp.threads;
        sp.lds = (sp.lds + 15) & ~(size_t) 15;
        if (sp.lds <= lds_max) { sp.ncol = sp.threads; break; }
    }
    if (!sp.ncol) { // very large sketches: one wave, as many item lanes as columns fit
        sp.threads = 64;
        const size_t fixed = (size_t) 16 * m + (size_t) 8 * chunk + 16 + 16;
        if (fixed < lds_max) sp.ncol = (int) std::min<size_t>(64, (lds_max - fixed) / (pt * (size_t) m));
        sp.lds = (fixed + pt * (size_t) m * sp.ncol + 15) & ~(size_t) 15;
    }
    sp.blocks_per_cu = std::max<int>(1, std::min<int>(2048 / sp.threads, (int) (lds_max / sp.lds)));
    return sp;
}

// n lists of pre-hashed values as "sequences": list i = vals[offsets[i] .. offsets[i + 1]) (the launchers get `vals` as `hashed` too)
inline DevSeqs hashed_seqs(const void *vals, const uint64_t *offsets, uint32_t n) {
    DevSeqs ds;
    ds.bases = reinterpret_cast<const uint8_t *>(vals);
    ds.offsets = offsets;
    ds.n_seq = n;
    ds.total_bytes = 1; // unused for pre-hashed input
    return ds;
}

// ---- kmu_sketch_super.hip, kmu_sketch_dens.hip ----
int launch_super(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const void *hashed,
                 int hashed_bytes, uint64_t *part_rows);
int launch_super_reduce(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *part_rows, uint64_t n_parts, void *d_sig);
int launch_dens(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const void *hashed,
                int hashed_bytes);
int launch_dens_merge(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *parts, uint32_t n_parts, void *d_sig);

// ---- kmu_sketch_pmh.hip ----
// What a launch_pmh3a call sketches besides the sequences of `ds`; every field may stay at its default.
struct PmhInputs {
    const uint64_t *d_block_rows = nullptr; // block mode: row offsets per read
    uint32_t *d_counts = nullptr;           // bottom-k counts, or null
    const void *hashed = nullptr;           // pre-hashed values (hashed_bytes = 4 / 8 each) instead of bases
    int hashed_bytes = 0;
    uint64_t *part_h = nullptr, *part_k = nullptr; // slot minima per "sequence" instead of signature rows
    uint32_t skip_longer = 0;               // sequences with more k-mers are left to the global (partitioned) route
    const uint64_t *len_stats = nullptr;    // longest sequence, all bases (whole sequences only), or null
};
int launch_pmh3a(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err,
                 const PmhInputs &in = PmhInputs());
// ProbMinHash3a slot minima (part_h, part_k: n_leaves rows) of n_leaves lists of pre-hashed u64 values, list i = items[bounds[i] .. bounds[i + 1])
int launch_pmh3a_leaves(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *items, const uint64_t *bounds, uint32_t n_leaves,
                        uint64_t *part_h, uint64_t *part_k, uint32_t *d_err);
// ProbMinHash3a, one signature per sequence, sequences on the device.  h_offsets: a host copy of ds.offsets[0 .. n_seq] if the
// caller has one (the lengths are then known without asking the device), else null.
int sketch_pmh_per_seq(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_block_rows, void *d_sig,
                       uint32_t *d_err, const uint64_t *h_offsets);

// ---- kmu_sketch.hip ----
// *p: the resolved parameters of an entry point that sketches sequences of `input_kind`, after its checks: resolve_algo,
// check_kmer, the sketch parameters, check_fhash_input -- in this order
int sketch_seq_params(kmu_ctx *ctx, const kmu_sketch_params *p_in, int input_kind, kmu_sketch_params *p);
// sketch_seq_params, then "no bottom-k over a list of sequences": the checks kmu_sketch and kmu_sketch_groups share
int sketch_params(kmu_ctx *ctx, const kmu_sketch_params *p_in, kmu_sketch_params *p);
// k_nk_scan: the k-mer offsets of the sequences of ds into "all.koff" ((*koff)[n_seq]: their total).  No host synchronisation.
int launch_nk_scan(kmu_ctx *ctx, const DevSeqs &ds, int kmer_size, uint32_t *d_err, const uint64_t **koff);
// launch_nk_scan and the total read back: one device-to-host copy, one synchronisation
int count_kmers(kmu_ctx *ctx, const DevSeqs &ds, int kmer_size, uint32_t *d_err, const uint64_t **koff, uint64_t *n_items);
// k_seq_hashes_compact: fhash of every k-mer of every sequence of ds, one after the other, to d_out (nothing when ds is empty)
int launch_hashes_compact(kmu_ctx *ctx, const DevSeqs &ds, const KmerCfg &cfg, const uint64_t *koff, uint64_t *d_out, uint32_t *d_err);
// count_kmers, "all.hashes" sized for them, launch_hashes_compact into it
int hash_all_kmers(kmu_ctx *ctx, const DevSeqs &ds, const KmerCfg &cfg, uint32_t *d_err, const uint64_t **koff, const uint64_t **hashes,
                   uint64_t *n_items);
// One sketch over a device array of n pre-hashed values (u64, zero-extended Kmer::Val)
int sketch_all_hashed(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *d_vals, uint64_t n, void *d_sig, uint32_t *d_err);
// per-sequence signatures of device-resident sequences for any algorithm.  d_block_rows: ProbMinHash3a block mode, else null;
// d_counts: bottom-k counts, or null
int sketch_per_seq_device(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_block_rows, uint32_t *d_counts,
                          void *d_sig, uint32_t *d_err, const uint64_t *h_offsets);

} // namespace kmu

// kmu_sketch_dens.h -- what the two users of the bins / registers sketches share: kmu_sketch_dens.hip (kmu_sketch, kmu_sketch_hashed,
// the partials) and kmu_sketch_groups.hip (the batched route of kmu_sketch_groups).  The argument block, the device functions that
// walk a sequence, update, densify, merge and store a row, and the host steps that fill the block and size its LDS.  The comments on
// the algorithms and their device mapping are at the top of kmu_sketch_dens.hip.
#pragma once

#include "kmu_sketch_host.hpp"
#include "kmu_stream.h"

namespace kmu {

struct DensArgs {
    const uint8_t *bases;
    const uint64_t *offsets;
    const uint64_t *packed_offsets;
    uint32_t n_seq;
    int packed;
    uint64_t total_bytes;
    KmerCfg cfg;
    int m;
    int hasher;
    int rand08;
    int f32;      // signature is f32 (bins hold f32 bit patterns)
    int val_w32;  // Kmer::Val is 32 bits
    int rev;      // reverse densification
    int hll;      // SetSketch registers instead of bins: maxima of k = floor(1 - log_b x), no densification
    int sig_bytes; // 2 / 4 / 8: width of a signature entry
    uint32_t q;   // SetSketch: registers are clamped to [0, q + 1]
    double inv_am, inv_ln_b; // SetSketch: 1 / (a m), 1 / ln b
    uint32_t idx_thresh;  // rand 0.9 Uniform<usize>(0, m): reject while lo < (2^32 - m) % m
    uint64_t idx_zone;    // rand 0.8 Uniform<usize>(0, m): accept while lo <= zone
    const void *hashed; // pre-hashed input (offsets count values), else null
    int hashed_bytes;
    uint32_t skip_longer; // sequences with more k-mers are left to k_oph_long
    uint32_t long_seq;    // k_oph_long: the sequence to walk
    uint64_t *row;        // global accumulation row (m bit patterns), k_oph_reads<true> / k_oph_long / k_oph_finish
    uint64_t out_row;     // k_oph_finish: signature row to write
    void *sig_out;
    uint32_t *queue;
    uint32_t *err;
};

__device__ __forceinline__ uint64_t oph_large_bits(int f32) {
    return f32 ? (uint64_t) __float_as_uint(4294967296.0f) : (uint64_t) __double_as_longlong(4294967295.0); // F::from(u32::MAX)
}

// h(bin, attempt) in [0, m): SplitMix64 finaliser of the pair, reduced by multiply-high (this implementation's choice)
__device__ __forceinline__ uint32_t dens_hash(uint32_t bin, uint32_t attempt, uint32_t m) {
    uint64_t z = (((uint64_t) bin << 32) | attempt) + 0x9e3779b97f4a7c15ull;
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    z ^= z >> 31;
    return (uint32_t) __umul64hi(z, (uint64_t) m);
}

__device__ __forceinline__ SeqView dens_view(const DensArgs &a, uint32_t r) {
    SeqView sv;
    sv.base = a.bases;
    sv.len = a.offsets[r + 1] - a.offsets[r];
    sv.packed = a.packed;
    if (a.packed) {
        sv.begin = a.packed_offsets[r];
        sv.total = a.total_bytes ? a.total_bytes
                                 : (a.packed_offsets[a.n_seq - 1] + (a.offsets[a.n_seq] - a.offsets[a.n_seq - 1] + 3) / 4);
    } else {
        sv.begin = a.offsets[r];
        sv.total = a.total_bytes ? a.total_bytes : a.offsets[a.n_seq];
    }
    return sv;
}

// Uniform<usize>(0, m) with the rejection bounds computed once on the host (the sketch size is fixed for the launch)
__device__ __forceinline__ uint32_t dens_draw_bin(const DensArgs &a, Xoshiro &rng) {
    if (a.rand08) {
        for (;;) {
            const uint64_t v = rng.next();
            const uint64_t hi = __umul64hi(v, (uint64_t) a.m), lo = v * (uint64_t) a.m;
            if (lo <= a.idx_zone) return (uint32_t) hi;
        }
    }
    for (;;) {
        const uint64_t mm = (uint64_t) rng.next_u32() * (uint32_t) a.m;
        if ((uint32_t) mm >= a.idx_thresh) return (uint32_t) (mm >> 32);
    }
}

// natural logarithm of a positive normal double from +, -, *, / only (the oracle carries the same few lines): x = 2^e f with
// f in (sqrt(1/2), sqrt(2)], log f = 2 s (1 + z/3 + ... + z^10/21), s = (f - 1) / (f + 1), z = s^2
__device__ __forceinline__ double kmu_log(double x) {
    uint64_t bits = (uint64_t) __double_as_longlong(x);
    int e = (int) ((bits >> 52) & 0x7FF) - 1023;
    double f = __longlong_as_double((long long) ((bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull));
    if (f > 1.4142135623730951) { f = f * 0.5; e += 1; }
    const double s = (f - 1.0) / (f + 1.0), z = s * s;
    double poly = 1.0 / 21.0;
    poly = poly * z + 1.0 / 19.0;
    poly = poly * z + 1.0 / 17.0;
    poly = poly * z + 1.0 / 15.0;
    poly = poly * z + 1.0 / 13.0;
    poly = poly * z + 1.0 / 11.0;
    poly = poly * z + 1.0 / 9.0;
    poly = poly * z + 1.0 / 7.0;
    poly = poly * z + 1.0 / 5.0;
    poly = poly * z + 1.0 / 3.0;
    poly = poly * z + 1.0;
    return (double) e * 0.6931471805599453 + 2.0 * s * poly;
}

// K_low of this workgroup's registers, refreshed by one wave (registers only grow, so the word only grows).
// Every lane of the wave calls this (uniform control flow).
__device__ __forceinline__ void hll_refresh_klow(const DensArgs &a, const uint64_t *hs, uint32_t *klow) {
    uint64_t mn = ~0ull;
    for (int i = lane_id(); i < a.m; i += 64) {
        const uint64_t v = __hip_atomic_load(&hs[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // (not volatile: that becomes a FLAT load)
        mn = v < mn ? v : mn;
    }
    mn = ~wave_max_u64(~mn);
    if (lane_id() == 0) atomicMax(klow, (uint32_t) mn);
}

// SetSketch (Ertl 2021, Algorithm 1, SetSketch1), one element per lane (`have`), the wave in lock step: ascending
// x_j = x_{j-1} + Exp(1) / (a m); k = clamp(floor(1 - log_b x_j)); a lane stops at its first k <= K_low (any lower bound of
// this workgroup's registers: later k are no larger); else a uniformly drawn register takes max(K_i, k).  While the
// registers are young every element runs long, so K_low is refreshed inside the loop (all lanes take part).
__device__ __forceinline__ void hll_wave_items(const DensArgs &a, uint64_t *hs, uint32_t *klow, bool have, uint64_t value) {
    Xoshiro rng;
    rng.s0 = rng.s1 = rng.s2 = rng.s3 = 0;
    if (have) rng.seed(hasher_finish(a.hasher, value, a.val_w32 != 0));
    double x = 0.0;
    int j = 0;
    uint32_t round = 0;
    bool active = have;
    while (__any(active)) {
        if (active) {
            x += -kmu_log(1.0 - rng.unif01()) * a.inv_am;
            const double t = 1.0 - kmu_log(x) * a.inv_ln_b;
            uint32_t k = 0;
            if (t >= (double) a.q + 1.0) k = a.q + 1u;
            else if (t > 0.0) k = (uint32_t) t;
            if (k <= __hip_atomic_load(klow, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) active = false;
            else {
                const uint32_t i = dens_draw_bin(a, rng);
                atomicMax((unsigned long long *) &hs[i], (unsigned long long) k);
                if (++j >= a.m) active = false;
            }
        }
        if ((++round & 31u) == 0u) hll_refresh_klow(a, hs, klow);
    }
}

// one item: r and bin from its own RNG stream, minimum into the bin
__device__ __forceinline__ void oph_item(const DensArgs &a, uint64_t *hs, uint64_t value) {
    Xoshiro rng;
    rng.seed(hasher_finish(a.hasher, value, a.val_w32 != 0));
    uint64_t bits;
    if (a.f32) bits = (uint64_t) __float_as_uint(rng.unif01_f32());
    else bits = (uint64_t) __double_as_longlong(rng.unif01());
    const uint32_t k = dens_draw_bin(a, rng);
    atomicMin((unsigned long long *) &hs[k], (unsigned long long) bits);
}

// the steps of a sequence: 64 code words (1024 bases) each, amino acids 64 residues each.  All words: the tail that starts no
// k-mer is validated too
__device__ __forceinline__ uint64_t oph_steps(const SeqView &sv, bool aa) {
    return aa ? (sv.len + 63) / 64 : (seq_num_words(sv) + 63) / 64;
}

// the items of the steps of one sequence, waves striding by `stride` steps from `first`, up to step st_end (or the last)
// (HLL: compile-time, so that the bins kernels do not carry the registers of the SetSketch loop)
template <bool HLL>
__device__ __forceinline__ uint32_t oph_walk(const DensArgs &a, const SeqView &sv, uint64_t *hs, uint32_t *klow, bool aa,
                                             uint64_t nk, uint64_t first, uint64_t stride, uint64_t st_end = ~0ull) {
    uint32_t bad = 0;
    if constexpr (HLL) {
        // the values of a step are collected first (the visit is per lane and per position), then worked off slot by slot
        // with the whole wave in step -- hll_wave_items needs uniform control flow
        if (a.hashed_bytes) {
            for (uint64_t p0 = first * 64; p0 < nk; p0 += stride * 64) {
                const uint64_t p = p0 + lane_id();
                uint64_t v = 0;
                if (p < nk)
                    v = a.hashed_bytes == 4 ? (uint64_t) reinterpret_cast<const uint32_t *>(a.hashed)[sv.begin + p]
                                            : reinterpret_cast<const uint64_t *>(a.hashed)[sv.begin + p];
                hll_wave_items(a, hs, klow, p < nk, v);
                if (((p0 / (stride * 64)) & 15u) == 15u) hll_refresh_klow(a, hs, klow);
            }
            return 0;
        }
        const uint64_t n_st = oph_steps(sv, aa), st1 = n_st < st_end ? n_st : st_end;
        for (uint64_t st = first; st < st1; st += stride) {
            uint64_t vals[16];
            uint32_t mask = 0;
            if (aa) {
                bad |= wave_step_kmers_aa(sv, a.cfg.k, st, 0, nk, [&](uint64_t, uint64_t val, uint64_t rc) {
                    vals[0] = apply_fhash(a.cfg, val, rc);
                    mask = 1u;
                });
            } else {
                const uint64_t p0 = (st * 64 + (uint64_t) lane_id()) * 16; // position + lead of this lane's first base
                const uint32_t lead = seq_lead(sv);
                bad |= wave_step_kmers(sv, a.cfg.k, st, 0, nk, [&](uint64_t pos, uint64_t val, uint64_t rc) {
                    const uint32_t slot = (uint32_t) (pos + lead - p0);
                    vals[slot] = apply_fhash(a.cfg, val, rc);
                    mask |= 1u << slot;
                });
            }
#pragma unroll
            for (int slot = 0; slot < 16; slot++) {
                if (!__any(mask >> slot & 1u)) continue; // uniform
                hll_wave_items(a, hs, klow, (mask >> slot & 1u) != 0u, vals[slot]);
            }
            hll_refresh_klow(a, hs, klow);
        }
        return bad;
    }
    auto visit = [&](uint64_t, uint64_t val, uint64_t rc) { oph_item(a, hs, apply_fhash(a.cfg, val, rc)); };
    if (a.hashed_bytes) {
        for (uint64_t p = first * 64 + lane_id(); p < nk; p += stride * 64) {
            const uint64_t v = a.hashed_bytes == 4 ? (uint64_t) reinterpret_cast<const uint32_t *>(a.hashed)[sv.begin + p]
                                                   : reinterpret_cast<const uint64_t *>(a.hashed)[sv.begin + p];
            oph_item(a, hs, v);
        }
    } else {
        const uint64_t n_st = oph_steps(sv, aa), st1 = n_st < st_end ? n_st : st_end;
        if (aa)
            for (uint64_t st = first; st < st1; st += stride) bad |= wave_step_kmers_aa(sv, a.cfg.k, st, 0, nk, visit);
        else
            for (uint64_t st = first; st < st1; st += stride) bad |= wave_step_kmers(sv, a.cfg.k, st, 0, nk, visit);
    }
    return bad;
}

// Densification of hs[0, m) in LDS by the whole workgroup.  filled: bitmap words; claim: m words (RevOptDens), all ones on
// entry and on exit; cnt: two words.  Every thread of the workgroup calls this.
__device__ __forceinline__ void oph_densify(const DensArgs &a, uint64_t *hs, uint32_t *filled, uint32_t *claim, uint32_t *cnt) {
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const uint32_t m = (uint32_t) a.m;
    const uint64_t large = oph_large_bits(a.f32);
    const uint32_t nwords = (m + 31) / 32;
    if (tid == 0) cnt[0] = 0;
    __syncthreads();
    uint32_t mine = 0;
    for (uint32_t w = tid; w < nwords; w += nthreads) {
        uint32_t bits = 0;
        for (uint32_t b = 0; b < 32 && w * 32 + b < m; b++) bits |= (hs[w * 32 + b] != large ? 1u : 0u) << b;
        filled[w] = bits;
        mine += (uint32_t) __popc(bits);
    }
    if (mine) atomicAdd(&cnt[0], mine);
    __syncthreads();
    const uint32_t n_filled = cnt[0];
    if (n_filled == 0 || n_filled == m) return; // nothing to copy from / nothing to fill (uniform)
    auto is_filled = [&](uint32_t j) { return (filled[j >> 5] >> (j & 31)) & 1u; };
    if (!a.rev) {
        for (uint32_t i = tid; i < m; i += nthreads) {
            if (is_filled(i)) continue;
            for (uint32_t attempt = 1;; attempt++) {
                const uint32_t j = dens_hash(i, attempt, m);
                if (is_filled(j)) { hs[i] = hs[j]; break; } // hs[j] of a filled bin never changes here
            }
        }
        __syncthreads();
        return;
    }
    uint32_t left = m - n_filled; // uniform
    for (uint32_t round = 1; left > 0; round++) {
        if (tid == 0) cnt[1] = 0;
        // offers: the smallest offering bin wins an empty target (the sequential sweep visits j in increasing order)
        for (uint32_t j = tid; j < m; j += nthreads) {
            if (!is_filled(j)) continue;
            const uint32_t i = dens_hash(j, round, m);
            if (hs[i] == large) atomicMin(&claim[i], j);
        }
        __syncthreads();
        uint32_t got = 0;
        for (uint32_t j = tid; j < m; j += nthreads) {
            if (!is_filled(j)) continue;
            const uint32_t i = dens_hash(j, round, m);
            if (claim[i] == j) { hs[i] = hs[j]; got++; } // exactly one offering bin sees its own index
        }
        if (got) atomicAdd(&cnt[1], got);
        __syncthreads();
        for (uint32_t j = tid; j < m; j += nthreads) { // wipe the claims of this round
            if (!is_filled(j)) continue;
            claim[dens_hash(j, round, m)] = 0xFFFFFFFFu;
        }
        left -= cnt[1];
        __syncthreads();
    }
}

__device__ __forceinline__ void oph_store_row(const DensArgs &a, const uint64_t *hs, uint64_t row) {
    for (int t = threadIdx.x; t < a.m; t += blockDim.x) {
        if (a.sig_bytes == 2) reinterpret_cast<uint16_t *>(a.sig_out)[row * a.m + t] = (uint16_t) hs[t];
        else if (a.sig_bytes == 4) reinterpret_cast<uint32_t *>(a.sig_out)[row * a.m + t] = (uint32_t) hs[t];
        else reinterpret_cast<uint64_t *>(a.sig_out)[row * a.m + t] = hs[t];
    }
}

// neutral element of a bin / register, and the merge of a workgroup's array into the global row
__device__ __forceinline__ uint64_t oph_neutral(const DensArgs &a) { return a.hll ? 0ull : oph_large_bits(a.f32); }
__device__ __forceinline__ void oph_merge_to_row(const DensArgs &a, const uint64_t *hs) {
    const uint64_t neutral = oph_neutral(a);
    for (int s = threadIdx.x; s < a.m; s += blockDim.x) {
        if (hs[s] == neutral) continue;
        if (a.hll) atomicMax((unsigned long long *) &a.row[s], (unsigned long long) hs[s]);
        else atomicMin((unsigned long long *) &a.row[s], (unsigned long long) hs[s]);
    }
}

// LDS layout shared by the kernels: hs[m] | filled[(m + 31) / 32] | cnt[4] | claim[m] (RevOptDens only)
__device__ __forceinline__ void oph_lds(const DensArgs &a, uint8_t *smem, uint64_t *&hs, uint32_t *&filled, uint32_t *&cnt,
                                        uint32_t *&claim) {
    hs = reinterpret_cast<uint64_t *>(smem);
    filled = reinterpret_cast<uint32_t *>(hs + a.m);
    cnt = filled + (a.m + 31) / 32;
    claim = cnt + 4;
}

// ---- host (kmu_sketch_dens.hip) ----
static constexpr size_t DENS_LDS_MAX = 160 * 1024;    // dynamic LDS a workgroup of these kernels may ask for
// the argument block of a call: input, parameters, rejection bounds, the context's SetSketchParams; row / queue / modes stay zero
void dens_args(const kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const void *hashed,
               int hashed_bytes, DensArgs *a);
// oph_neutral on the host: F::from(u32::MAX) as f64 / f32, zero registers
inline uint64_t dens_neutral_bits(const DensArgs &a) { return a.hll ? 0ull : super_init_bits(a.f32 ? 1 : 0); }
// bytes of oph_lds' layout
inline size_t dens_lds_full(const DensArgs &a) {
    return ((size_t) 8 * a.m + 4 * ((size_t) (a.m + 31) / 32) + 16 + (a.rev ? (size_t) 4 * a.m : 0) + 15) & ~(size_t) 15;
}
// KMU_E_UNSUPPORTED if that layout does not fit the LDS; above 64 KiB the kernels `fns` are allowed DENS_LDS_MAX
int dens_lds_check(kmu_ctx *ctx, const DensArgs &a, const void *const *fns, int n_fns);

} // namespace kmu

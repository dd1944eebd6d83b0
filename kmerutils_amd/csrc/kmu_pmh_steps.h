// kmu_pmh_steps.h -- the device steps that two or more of the sketch kernel files share (kmu_pmh_general.hip, kmu_pmh_uq.hip,
// kmu_pmh_long.hip, kmu_pmh_short.hip, kmu_pmh_smallk.hip, kmu_pmh_points.hip): the slot minima and their q_max, the ProbMinHash3a point process of a key,
// how reads are taken from the queue, the view of a queue entry, a k-mer out of staged code words.  A step only one file uses lives there.
#pragma once

#include "kmu_sketch_kernels.h"
#include "kmu_stream.h"

namespace kmu {

static constexpr uint64_t H_INIT = 0x7FEFFFFFFFFFFFFFull;    // bits of f64::MAX (MaxValueTracker initial value)
static constexpr uint64_t H_BUSY = 0xFFFFFFFFFFFFFFFEull;    // slot being updated

__device__ __forceinline__ uint32_t mix32(uint64_t key) {
    uint32_t x = (uint32_t) key ^ (uint32_t) (key >> 32);
    x *= 0x9E3779B1u;
    x ^= x >> 15;
    return x;
}

// slot update: keep (h, key) minimal per slot; exact ties go to the smaller key (order independence)
__device__ __forceinline__ void slot_update(uint64_t *hmin, uint64_t *sig, uint32_t k, double h, uint64_t key) {
    const uint64_t hb = (uint64_t) __double_as_longlong(h);
    for (;;) {
        uint64_t cur = __hip_atomic_load(&hmin[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (cur == H_BUSY) continue;
        if (hb > cur) return;
        if (hb == cur && key >= __hip_atomic_load(&sig[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)) return;
        if (atomicCAS((unsigned long long *) &hmin[k], (unsigned long long) cur, (unsigned long long) H_BUSY) == cur) {
            __hip_atomic_store(&sig[k], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            __threadfence_block();
            atomicExch((unsigned long long *) &hmin[k], (unsigned long long) hb);
            return;
        }
    }
}

// the same for slot arrays that belong to ONE wave (k_pmh_points): the lanes of a call run in lock step, so the minimum
// is taken by one LDS atomic and the winner is whoever finds its own value there afterwards; no lock word, no loop.
// Lanes of a call that meet in a slot with the same h (and therefore the same `cur`) take the same branch below.
__device__ __forceinline__ void slot_update_wave(uint64_t *hmin, uint64_t *sig, uint32_t k, double h, uint64_t key) {
    const uint64_t hb = (uint64_t) __double_as_longlong(h);
    const uint64_t cur = __hip_atomic_load(&hmin[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    const bool cand = hb <= cur;
    if (cand) __hip_atomic_fetch_min(&hmin[k], hb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (cand && __hip_atomic_load(&hmin[k], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == hb) {
        if (hb < cur) __hip_atomic_store(&sig[k], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); // the old key is obsolete
        __hip_atomic_fetch_min(&sig[k], key, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);           // exact ties: smaller key
    }
}

// q_max = max over slots of the current minima (MaxValueTracker root); a slot in flight counts as "unknown" = MAX
__device__ __forceinline__ uint64_t wave_qmax(const uint64_t *hmin, int m) {
    uint64_t q = 0;
    for (int i = lane_id(); i < m; i += 64) {
        uint64_t v = __hip_atomic_load(&hmin[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        if (v == H_BUSY) v = H_INIT;
        q = v > q ? v : q;
    }
    return wave_max_u64(q);
}

__device__ __forceinline__ uint32_t draw_slot(const SketchArgs &a, Xoshiro &rng) {
    if (a.rand08) {
        for (;;) {
            // v * m as 96 bits (m < 2^32): two 32 x 32 -> 64 multiply-adds instead of a full 64 x 64 high product
            const uint64_t v = rng.next();
            const uint64_t p0 = (uint64_t) (uint32_t) v * (uint32_t) a.m;
            const uint64_t p1 = (uint64_t) (uint32_t) (v >> 32) * (uint32_t) a.m + (p0 >> 32);
            const uint64_t lo = (p1 << 32) | (uint32_t) p0;
            if (lo <= a.idx_zone) return (uint32_t) (p1 >> 32);
        }
    }
    for (;;) {
        uint64_t mm = (uint64_t) rng.next_u32() * (uint32_t) a.m;
        if ((uint32_t) mm >= a.idx_thresh) return (uint32_t) (mm >> 32);
    }
}

__device__ __forceinline__ uint64_t splitmix_at(uint64_t seed, uint64_t i) {
    uint64_t z = seed + i * 0x9e3779b97f4a7c15ull; // SplitMix64 is counter based: output i depends on seed + i*G only
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// the rejection part of ExpRestricted01::sample (reached with probability 1 - 1/c1)
__device__ __forceinline__ double exp01_rest(const Exp01 &e, Xoshiro &rng) {
    for (;;) {
        double x = rng.unif01();
        if (x < e.c2) return x;
        double y = 0.5 * rng.unif01();
        if (y > 1.0 - x) {
            x = 1.0 - x;
            y = 1.0 - y;
        }
        if (x <= e.c3 * (1.0 - y)) return x;
        if (e.c1 * y <= 1.0 - x) return x;
        if (y * e.c1 * e.lambda <= expm1_small(e.lambda * (1.0 - x))) return x;
    }
}

// the single kernel: wave w recomputes the workgroup's q_max when (chunk + w) % 16 == 0, i.e. one of the sixteen waves per
// chunk of 1024 keys, and posts it for the others (every 4: 88.7 ms, 8: 87.3, 16: 87.0 on the ONT workload)
static constexpr uint32_t B1_REFRESH_MASK = 15u;
__device__ __forceinline__ double winv_of(const double *lut, uint32_t w) {
    if (lut && w < WINV_LUT) return lut[w];
    return 1.0 / (double) w;
}
// an entry of that table: what winv_of computes without it (entry 0 is never looked at: a weight is at least 1)
__device__ __forceinline__ double winv_entry(uint32_t t) { return t ? 1.0 / (double) t : 0.0; }

// ProbMinHash3a, pass B1: the FIRST point of every key (h1 = winv * Exp01, slot k1).  Like the crate's first loop over
// the map, a key that may need further points (winv < q_max) is only remembered (return value) -- the crate pushes it
// to `to_be_processed` and comes back to it after every key had its first point, when q_max is small and most of
// those keys are dropped without drawing anything.  `qmax` is any upper bound of the current q_max (shared word,
// refreshed now and then); pruning with a stale bound never changes the arg-min.
// The first xoshiro256++ output needs only state words s0 and s3 (= SplitMix64 outputs 1 and 4 of the seed): the
// other two are computed only for the keys whose first point survives the q_max test.
__device__ __forceinline__ bool pmh3a_first_point(const SketchArgs &a, bool sig32, uint64_t *hmin, uint64_t *sig,
                                                  uint64_t *qmax_sh, bool refresh, bool have, uint64_t key, uint32_t w,
                                                  const double *winv_lut = nullptr) {
    uint64_t qb;
    if (refresh) {
        qb = wave_qmax(hmin, a.m);
        if (lane_id() == 0) atomicMin((unsigned long long *) qmax_sh, (unsigned long long) qb);
    } else {
        qb = __hip_atomic_load(qmax_sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    }
    bool deferred = false;
    if (have) {
        const uint64_t seed = hasher_finish(KMU_HASHER_NOHASH, key, sig32);
        const double winv = winv_of(winv_lut, w);
        Xoshiro rng;
        rng.s0 = splitmix_at(seed, 1);
        rng.s3 = splitmix_at(seed, 4);
        const uint64_t r1 = rotl64(rng.s0 + rng.s3, 23) + rng.s0;
        const double u1 = __longlong_as_double((long long) ((r1 >> 12) | 0x3FF0000000000000ull)) - 1.0;
        double x = a.e01.c1 * u1;
        const double qmax = __longlong_as_double((long long) qb);
        const bool slow = !(x < 1.0);
        if (slow || winv * x < qmax) {
            rng.s1 = splitmix_at(seed, 2);
            rng.s2 = splitmix_at(seed, 3);
            (void) rng.next(); // the draw already used
            if (slow) x = exp01_rest(a.e01, rng);
            const double h = winv * x;
            if (h < qmax) {
                uint32_t k = draw_slot(a, rng);
                slot_update(hmin, sig, k, h, key);
                deferred = winv < qmax; // the crate: `if winv < qmax { to_be_processed.push(..) }`
            }
        }
    }
    return deferred;
}

// pass B2: further points (rounds i >= 2) of the remembered keys, against the q_max reached after all first points.
// The RNG stream of a key is replayed from its seed: round 1 consumed the Exp01 draws and one slot draw.
// `qb` (bits of a q_max upper bound) is carried by the wave across calls and refreshed after every round.
template <bool WAVE_PRIVATE = false>
__device__ __forceinline__ void pmh3a_more_points(const SketchArgs &a, bool sig32, uint64_t *hmin, uint64_t *sig,
                                                  uint64_t &qb, bool alive, uint64_t key, double winv) {
    Xoshiro rng;
    uint32_t i = 2;
    if (alive) {
        rng.seed(hasher_finish(KMU_HASHER_NOHASH, key, sig32));
        (void) exp01_sample(a.e01, rng);
        (void) draw_slot(a, rng);
    }
    while (__any(alive)) {
        if (alive) {
            double qmax = __longlong_as_double((long long) qb);
            double hbase = winv * (double) (i - 1);
            if (!(hbase < qmax)) {
                alive = false;
            } else {
                double x = exp01_sample(a.e01, rng);
                double h = hbase + winv * x;
                uint32_t k = draw_slot(a, rng); // rounds >= 2 always draw the slot
                if (h < qmax) {
                    if (WAVE_PRIVATE) slot_update_wave(hmin, sig, k, h, key);
                    else slot_update(hmin, sig, k, h, key);
                }
                if (!(winv * (double) i < qmax)) alive = false;
                i++;
            }
        }
        qb = wave_qmax(hmin, a.m);
    }
}

// A word every thread reads from the same LDS address is the same in all lanes, but the compiler cannot know: taking it
// through readfirstlane puts it (and every loop bound, address and branch derived from it) on the scalar unit.
__device__ __forceinline__ uint32_t uniform_u32(uint32_t v) { return (uint32_t) __builtin_amdgcn_readfirstlane((int) v); }
__device__ __forceinline__ uint64_t uniform_u64(uint64_t v) {
    return ((uint64_t) uniform_u32((uint32_t) (v >> 32)) << 32) | uniform_u32((uint32_t) v);
}

// A wave that takes reads by itself: lane 0 keeps a cursor (q_next, q_end; both start at 0), takes QCHUNK reads per atomic and hands out
// one, to every lane and on the scalar unit -- one same-address atomic per read would cap the whole grid at the L2's rate for a single
// address.  The queue never runs dry: the caller stops at the first entry beyond its reads.
// (The cursor is two plain words of the caller, not a struct with this as a method: k_pmh_points keeps its instruction stream only so.)
__device__ __forceinline__ uint32_t wave_take(uint32_t *queue, uint32_t &q_next, uint32_t &q_end, int lane) {
    uint32_t r = 0;
    if (lane == 0) {
        if (q_next == q_end) {
            q_next = atomicAdd(queue, (uint32_t) QCHUNK);
            q_end = q_next + QCHUNK;
        }
        r = q_next++;
    }
    return uniform_u32(r);
}

// the view of sequence r of the call's input
__device__ __forceinline__ SeqView seq_view_of(const SketchArgs &a, uint32_t r) {
    // (the header words come back in vector registers although `r` is uniform: handing them to the scalar unit
    // keeps every length, bound and address derived from them off the vector ALU)
    SeqView v;
    v.base = a.bases;
    v.len = uniform_u64(a.offsets[r + 1] - a.offsets[r]);
    v.packed = a.packed;
    if (a.packed) {
        v.begin = uniform_u64(a.packed_offsets[r]);
        v.total = a.total_bytes ? a.total_bytes
                                : uniform_u64(a.packed_offsets[a.n_seq - 1] + (a.offsets[a.n_seq] - a.offsets[a.n_seq - 1] + 3) / 4);
    } else {
        v.begin = uniform_u64(a.offsets[r]);
        v.total = a.total_bytes ? a.total_bytes : uniform_u64(a.offsets[a.n_seq]);
    }
    return v;
}

// the k-mer that starts at base `qq` of the code words staged in LDS (16 bases each): cut out of a window of three words
__device__ __forceinline__ uint64_t staged_kmer(const uint32_t *words, uint32_t qq, int k) {
    const uint32_t idx = qq >> 4, sh = (qq & 15u) * 2u;
    const uint64_t hi = ((uint64_t) words[idx] << 32) | words[idx + 1];
    const uint64_t v = (hi << sh) | (((uint64_t) words[idx + 2] << sh) >> 32);
    return v >> (64 - 2 * k);
}

} // namespace kmu

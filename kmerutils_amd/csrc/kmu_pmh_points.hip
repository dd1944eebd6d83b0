// kmu_pmh_points.hip -- the points of the two-kernel ProbMinHash3a routes: k_pmh_points turns the (key, weight) lists the multiset
// kernels leave (kmu_pmh_general.hip <EMIT>, kmu_pmh_uq.hip, kmu_pmh_short.hip, kmu_pmh_smallk.hip <EMIT>) into signature rows;
// k_pmh_reduce merges the slot minima of partial sketches.
#include "kmu_pmh_steps.h"

namespace kmu {

// q_max of the wave's slots is recomputed every 16 chunks of 64 keys (every 4: 21.0 ms, 8: 20.0, 16: 19.8 on the ONT
// workload; a stale bound only lets a few more keys into the expensive half)
static constexpr uint32_t PTS_REFRESH_MASK = 15u;

// the cheap half of pmh3a_first_point: can the first point of this key lie below q_max (bits `qb`)?  Needs two of the four
// SplitMix64 words and one f64 product; the rare keys whose first Exp01 draw falls in the sampler's rejection branch pass.
// UNIT_W: every key of the call has weight 1 (a chunk inside the weight-1 prefix of a list): 1 / w = 1.0 needs no look-up
template <bool UNIT_W = false>
__device__ __forceinline__ bool pmh3a_first_point_may_matter(const SketchArgs &a, bool sig32, uint64_t qb, uint64_t key,
                                                             uint32_t w, const double *winv_lut, uint64_t &s0, uint64_t &s3) {
    const uint64_t seed = hasher_finish(KMU_HASHER_NOHASH, key, sig32);
    s0 = splitmix_at(seed, 1);
    s3 = splitmix_at(seed, 4);
    const uint64_t r1 = rotl64(s0 + s3, 23) + s0;
    const double u1 = __longlong_as_double((long long) ((r1 >> 12) | 0x3FF0000000000000ull)) - 1.0;
    const double x = a.e01.c1 * u1;
    if (UNIT_W) return !(x < 1.0) || x < __longlong_as_double((long long) qb);
    return !(x < 1.0) || winv_of(winv_lut, w) * x < __longlong_as_double((long long) qb);
}

// the other half, for a key that passed pmh3a_first_point_may_matter: s0 / s3 are the two state words it computed
// UNIT_W: every key of the call has weight 1 -- no look-up, and the point is x itself (x times 1.0 is x, bit for bit)
template <bool UNIT_W = false>
__device__ __forceinline__ void pmh3a_first_point_rest(const SketchArgs &a, bool sig32, uint64_t *hmin, uint64_t *sig,
                                                       const uint64_t *qmax_sh, bool have, uint64_t key, uint32_t w,
                                                       uint64_t s0, uint64_t s3, const double *winv_lut) {
    const uint64_t qb = __hip_atomic_load(qmax_sh, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (have) {
        const double winv = UNIT_W ? 1.0 : winv_of(winv_lut, w);
        const uint64_t r1 = rotl64(s0 + s3, 23) + s0;
        const double u1 = __longlong_as_double((long long) ((r1 >> 12) | 0x3FF0000000000000ull)) - 1.0;
        double x = a.e01.c1 * u1;
        const double qmax = __longlong_as_double((long long) qb);
        const bool slow = !(x < 1.0);
        if (slow || (UNIT_W ? x : winv * x) < qmax) { // (q_max may have fallen since the key was queued)
            const uint64_t seed = hasher_finish(KMU_HASHER_NOHASH, key, sig32);
            Xoshiro rng;
            rng.s0 = s0;
            rng.s3 = s3;
            rng.s1 = splitmix_at(seed, 2);
            rng.s2 = splitmix_at(seed, 3);
            (void) rng.next(); // the draw already used
            if (slow) x = exp01_rest(a.e01, rng);
            const double h = UNIT_W ? x : winv * x;
            if (h < qmax) slot_update_wave(hmin, sig, draw_slot(a, rng), h, key);
        }
    }
}

// ProbMinHash3a points from the (key, weight) lists of k_sketch_pmh3a<.., EMIT>: one WAVE per read, so there is no
// workgroup barrier anywhere and a CU holds as many reads in flight as its registers allow.  LDS per wave: the slot
// minima (16 m bytes) + the shared q_max word.  Pass 1 = first point of every key; pass 2 = further rounds for the keys
// with winv < q_max (a key is deferred in pass 1 exactly when winv < q_max then, and q_max only falls: re-testing
// against the settled q_max selects a subset of the deferred keys, those that can still produce a point below it).
// LONG reads (more than pts_long_t list entries; their indices are in pts_long: [0] count, [2..] indices, k_pts_long_list)
// come first and are taken by a whole WORKGROUP: its four waves walk every fourth chunk of the list with slot arrays of their
// own and the row is the per-slot minimum of the four (smaller h, then smaller key: the rule of slot_update_wave).  A wave
// prunes with the q_max of ITS minima, which is >= the q_max of the merged ones -- it only rejects points that cannot be a
// slot's minimum -- so the row is the one a single wave makes.  One wave does 4.6e4 k-mers per ms: a 200 kb read alone took
// 4.3 ms, twice what the kernel needs for a 512 MB chunk of the host leg.
__global__ void __launch_bounds__(256) k_pts_long_list(const uint32_t *lst_n, uint32_t n_seq, uint32_t thr, uint32_t *out) {
    const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r < n_seq && lst_n[r] > thr) out[2 + atomicAdd(&out[0], 1u)] = r;
}
// q_max over the minima of the four waves of a workgroup together (a long read's waves prune with it: a point at or above it
// cannot be the minimum of its slot in the merged row either; without it every wave fills all m slots from its quarter of the
// keys alone and the four make ~3x the accepted points of one wave)
__device__ __forceinline__ uint64_t wg4_qmax(const uint64_t *arrays, size_t wave_words, int m) {
    uint64_t q = 0;
    for (int t = lane_id(); t < m; t += 64) {
        uint64_t v = H_INIT;
#pragma unroll
        for (int w4 = 0; w4 < 4; w4++) {
            const uint64_t x = __hip_atomic_load(&arrays[(size_t) w4 * wave_words + t], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            v = x < v ? x : v;
        }
        q = v > q ? v : q;
    }
    return wave_max_u64(q);
}

// one read's points.  WG = false: by this wave alone (chunks 0, 64, 128, ...).  WG = true: by the four waves of the workgroup,
// wave w on chunks 64 w, 64 w + 256, ... with slot arrays of its own, the row = per-slot minimum of the four.
template <bool SIG32, bool WG>
__device__ __forceinline__ void pts_one_read(const SketchArgs &a, uint32_t r, uint8_t *smem, size_t wave_words, const double *winv_lut) {
    const int wave = threadIdx.x >> 6, lane = lane_id();
    constexpr bool sig32 = SIG32;
    constexpr uint32_t cstride = WG ? 256u : 64u;
    const uint32_t cstart = WG ? 64u * (uint32_t) wave : 0u;
    uint64_t *arrays = reinterpret_cast<uint64_t *>(smem);
    uint64_t *hmin = arrays + (size_t) wave * wave_words;
    uint64_t *sig = hmin + a.m;
    uint64_t *qmax_sh = sig + a.m;
    uint64_t *qk = qmax_sh + 2;
    uint32_t *qw = reinterpret_cast<uint32_t *>(qk + 128);
    uint64_t *qs0 = qk + 128 + 64, *qs3 = qs0 + 128; // the two xoshiro state words the cheap test computed
    const uint64_t base = a.offsets[r] - a.offsets[0];
    const uint32_t n = uniform_u32(a.lst_n[r]);
    const uint32_t n_u = uniform_u32(a.lst_nu[r]); // leading entries of weight 1 without a weight word
    // tau: an a-priori guess of an upper bound of the read's FINAL q_max.  The first point of a key of weight w lies below t with
    // probability ~ min(1, w t) (Exp01 at lambda = ln(m / (m - 1)) is almost uniform) in a uniformly drawn slot, so with W k-mer
    // occurrences in the read a slot stays without a point below t with probability ~ exp(-t W / m): tau = m (ln m + c) / W leaves
    // one of the m slots empty with probability ~ e^-c, and only ~ m (ln m + c) keys lie below it however long the read is -- the
    // running q_max lets ~ 1180 (1 + ln(n / 1180)) of n keys into the expensive half.  Pass 1 prunes with min(q_max, tau); the guess
    // is verified below, and a read it fails for is done again without it.  No bound (H_INIT) where tau >= 1, where the list has
    // fewer entries than the keys tau wants below it, and with the bound switched off (tau_min_n = 2^32 - 1).
    uint64_t tau_b = H_INIT;
    if (n >= a.tau_min_n) {
        const uint64_t len = a.offsets[r + 1] - a.offsets[r];
        const uint64_t kk = (uint64_t) a.cfg.k;
        const double tau = a.tau_num / (double) (len >= kk ? len - kk + 1 : 0); // (W from the read's length: non-ACGT is an error anyway)
        if (tau < 1.0) tau_b = (uint64_t) __double_as_longlong(tau);
        tau_b = uniform_u64(tau_b);
    }
    uint32_t wmax = n_u ? 1u : 0u; // largest weight this lane saw (the prefix's chunks do not look: a list with a prefix has a weight 1)
    uint64_t qb = H_INIT;
    for (int turn = 0; turn < 2; turn++) { // the second turn runs without tau: H_INIT bounds every q_max, it cannot fail
        for (int t = lane; t < a.m; t += 64) { hmin[t] = H_INIT; sig[t] = 0; }
        if (lane == 0) *qmax_sh = tau_b;
        if (WG) __syncthreads(); // (the other waves' arrays are looked at from the first refresh on)
        // ---- pass 1 ----
        uint32_t chunk = 0, qn = 0; // qn: queued pairs (uniform)
        qb = tau_b;
        // while tau bounds the pass, the running q_max lies above it for the first part of the list and a refresh there is clamped back
        // to tau: none before `hold` of this wave's chunks (PTS_TAU_HOLD; the turn without tau refreshes from its first chunk on)
        const uint32_t hold = tau_b != H_INIT && n > cstart ? (uint32_t) (((uint64_t) ((n - cstart + cstride - 1u) / cstride) * a.tau_hold) >> 8) : 0u;
        // (Round 5, measured and not kept: the keys of 2 / 4 / 8 chunks in flight instead of one -- 18.40 / 18.42 / 19.60 against 18.38 ms,
        //  profiles/r05_pts_ahead.txt.  With everything but the list walk switched off the kernel takes 9.3 ms -- 38 GB of lists at
        //  4.1 TB/s -- but the whole kernel is bound by instruction issue: 1.008e10 vector wave-instructions at the half-rate peak are
        //  18 ms, the walk's loads are under them already; profiles/r05_pts_parts.txt.)
        uint64_t key_nx = 0; // the next chunk's pair is requested one iteration ahead
        uint32_t w_nx = 1;
        {
            const uint32_t i = cstart + (uint32_t) lane;
            if (i < n) { key_nx = a.lst_keys[base + i]; w_nx = i < n_u ? 1u : a.lst_w[base + i]; }
        }
        // The chunks that lie wholly inside the weight-1 prefix (c + 64 <= n_u; WG: this wave's own) are walked without weights: every
        // lane has an entry, its weight is 1, a survivor is queued without a weight word and worked off with h = x.  The general form
        // takes the rest, from the chunk that straddles n_u on; chunk counter, refresh cadence and the queue run on across both.
        uint32_t c = cstart;
        auto step = [&](auto unit_tag) __attribute__((always_inline)) {
            constexpr bool UNIT = decltype(unit_tag)::value;
            const uint32_t i = c + (uint32_t) lane;
            const uint64_t key = key_nx;
            const uint32_t w = UNIT ? 1u : w_nx;
            const bool have = UNIT || (i < n && w != 0u); // weight 0: a repeat of an earlier entry
            if (!UNIT && have) wmax = w > wmax ? w : wmax;
            if (i + cstride < n) key_nx = a.lst_keys[base + i + cstride];
            if (!UNIT) w_nx = 1u; // (UNIT: it is 1 since the walk began)
            if (c + cstride + 64u > n_u) { // (uniform: the next chunk reaches beyond the weight-1 prefix)
                if (i + cstride < n && i + cstride >= n_u) w_nx = a.lst_w[base + i + cstride];
            }
            // (WG: the four waves advance through the list together, so the merged q_max is refreshed four times as often per own
            //  chunk while it still falls fast -- the first 64 own chunks -- and at the single wave's cadence per own chunk after that)
            if ((chunk & (WG && chunk < 64u ? PTS_REFRESH_MASK >> 2 : PTS_REFRESH_MASK)) == 0u && chunk >= hold) {
                qb = WG ? wg4_qmax(arrays, wave_words, a.m) : wave_qmax(hmin, a.m);
                qb = qb < tau_b ? qb : tau_b;
                if (lane == 0) *qmax_sh = qb;
            }
            uint64_t s0 = 0, s3 = 0;
            const bool pass = have && pmh3a_first_point_may_matter<UNIT>(a, sig32, qb, key, w, winv_lut, s0, s3);
            const uint64_t pm = __ballot(pass);
            if (pass) {
                const uint32_t pos = qn + (uint32_t) __popcll(pm & ((1ull << lane) - 1ull));
                qk[pos] = key;
                if (!UNIT) qw[pos] = w;
                qs0[pos] = s0;
                qs3[pos] = s3;
            }
            qn += (uint32_t) __popcll(pm);
            if (qn >= 64u) { // the newest 64
                qn -= 64u;
                pmh3a_first_point_rest<UNIT>(a, sig32, hmin, sig, qmax_sh, true, qk[qn + lane], UNIT ? 1u : qw[qn + lane], qs0[qn + lane],
                                             qs3[qn + lane], winv_lut);
            }
        };
        for (; c + 64u <= n_u; c += cstride, chunk++) step(std::true_type{}); // uniform trip counts
        // (the prefix's survivors still queued get their weight word now, once per read, and leave with the next full 64: a flush here
        //  would run the expensive half with a partly filled wave)
        if ((uint32_t) lane < qn) qw[lane] = 1u;
        for (; c < n; c += cstride, chunk++) step(std::false_type{});
        if (qn) {
            const bool have = (uint32_t) lane < qn;
            pmh3a_first_point_rest(a, sig32, hmin, sig, qmax_sh, have, have ? qk[lane] : 0ull, have ? qw[lane] : 1u, have ? qs0[lane] : 0ull,
                                   have ? qs3[lane] : 0ull, winv_lut);
        }
        // ---- the true q_max after all first points; tau held if every slot has a point below it (an empty slot is H_INIT) ----
        if (WG) {
            __syncthreads(); // every wave's first points are in
            qb = wg4_qmax(arrays, wave_words, a.m);
        } else qb = wave_qmax(hmin, a.m);
        // (every pruned point lay at or above min(running q_max, tau) >= this q_max: none of them is a slot's minimum.  WG: the
        //  four waves decide alike -- a wave that goes on to pass 2 only lowers minima, one that starts over waits at the barrier)
        if (tau_b == H_INIT || qb < tau_b) break;
        tau_b = H_INIT;
        if (lane == 0 && (!WG || wave == 0)) atomicAdd(a.tau_redo, 1u);
        if (WG) __syncthreads(); // (nobody is still looking at the arrays that are wiped now)
    }
    // ---- pass 2 ----
    // (only a key with 1 / w < q_max draws again: with the largest weight of the read at hand the lists are read a
    //  second time only where that can happen at all.  Every key is tested again against the settled q_max and its generator is
    //  replayed from the seed: nothing here depends on which keys pass 1 worked off)
    wmax = (uint32_t) wave_max_u64((uint64_t) wmax);
    if (n && wmax && winv_of(winv_lut, wmax) < __longlong_as_double((long long) qb)) {
        // (a key of weight 1 draws again only while q_max > 1: with every slot hit q_max < 1 -- Exp01 is restricted to
        //  [0, 1) -- and the weight-1 prefix of the list is not read a second time)
        const uint32_t c0 = 1.0 < __longlong_as_double((long long) qb) ? 0u : (n_u & ~63u);
        uint32_t c = cstart;
        if (c < c0) c += (c0 - c + cstride - 1u) / cstride * cstride; // this wave's first chunk at or behind c0
        for (; c < n; c += cstride) {
            const uint32_t i = c + (uint32_t) lane;
            double winv = 0.0;
            bool alive = false;
            if (i < n) {
                const uint32_t w = i < n_u ? 1u : a.lst_w[base + i];
                winv = winv_of(winv_lut, w);
                alive = w != 0u && winv < __longlong_as_double((long long) qb);
            }
            if (__any(alive)) pmh3a_more_points<true>(a, sig32, hmin, sig, qb, alive, alive ? a.lst_keys[base + i] : 0ull, winv);
        }
    }
    // ---- signature row: arg-min key per slot, initobj (0) for an empty multiset ----
    if (WG) {
        __syncthreads();
        for (int t = threadIdx.x; t < a.m; t += 256) {
            uint64_t bh = arrays[t], bk = arrays[a.m + t];
#pragma unroll
            for (int w4 = 1; w4 < 4; w4++) { // smaller h, then smaller key: slot_update_wave's rule
                const uint64_t h = arrays[(size_t) w4 * wave_words + t], kk = arrays[(size_t) w4 * wave_words + a.m + t];
                if (h < bh || (h == bh && kk < bk)) { bh = h; bk = kk; }
            }
            const uint64_t v = bh == H_INIT ? 0ull : bk;
            if (sig32) reinterpret_cast<uint32_t *>(a.sig_out)[(uint64_t) r * a.m + t] = (uint32_t) v;
            else reinterpret_cast<uint64_t *>(a.sig_out)[(uint64_t) r * a.m + t] = v;
        }
        __syncthreads(); // (the arrays are wiped for the next read behind it)
    } else {
        for (int t = lane; t < a.m; t += 64) {
            const uint64_t v = hmin[t] == H_INIT ? 0ull : sig[t];
            if (sig32) reinterpret_cast<uint32_t *>(a.sig_out)[(uint64_t) r * a.m + t] = (uint32_t) v;
            else reinterpret_cast<uint64_t *>(a.sig_out)[(uint64_t) r * a.m + t] = v;
        }
    }
}

template <bool SIG32>
__global__ void __launch_bounds__(256) k_pmh_points(SketchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int lane = lane_id();
    // per wave: slot minima, arg-min keys, q_max word, and a queue of 128 (key, weight) pairs that passed the cheap test:
    // they are worked off 64 at a time, so the expensive half of a first point always runs with all lanes busy
    const size_t wave_words = 2 * (size_t) a.m + PTS_WAVE_WORDS;
    double *winv_lut = reinterpret_cast<double *>(reinterpret_cast<uint64_t *>(smem) + (size_t) 4 * wave_words);
    for (uint32_t t = threadIdx.x; t < WINV_LUT; t += blockDim.x) winv_lut[t] = winv_entry(t);
    __syncthreads();
    // the long reads first, a workgroup each (workgroup b: entries b, b + grid, ... of the list)
    // (only where a long read would be a tail: with more than four of them per workgroup of the grid they balance among themselves
    //  as single waves' reads, and the workgroup form costs more per key -- three barriers per read, q_max over four arrays)
    uint32_t n_long = a.pts_long ? a.pts_long[0] : 0u;
    if (n_long > 4u * gridDim.x) n_long = 0u;
    for (uint32_t li = blockIdx.x; li < n_long; li += gridDim.x) pts_one_read<SIG32, true>(a, a.pts_long[2 + li], smem, wave_words, winv_lut);
    uint32_t q_next = 0, q_end = 0; // lane 0's cursor into the queue (wave_take)
    for (;;) {
        const uint32_t r = wave_take(a.queue2, q_next, q_end, lane);
        if (r >= a.n_seq) break;
        if (n_long && uniform_u32(a.lst_n[r]) > a.pts_long_t) continue; // (taken by a workgroup above)
        pts_one_read<SIG32, false>(a, r, smem, wave_words, winv_lut);
    }
}

// merge the slot minima of disjoint key sets (leaves): per slot the smallest (h, key); one workgroup per slot
// (stride: words between the rows of consecutive parts; part_out: write (h, key) to part_out[t], part_out[m + t] instead)
__global__ void __launch_bounds__(256) k_pmh_reduce(const uint64_t *part_h, const uint64_t *part_k, uint64_t n_parts, int m,
                                                    uint64_t stride, int sig_bytes, void *sig_out, uint64_t *part_out) {
    __shared__ uint64_t sh[256], sk[256];
    const int t = blockIdx.x;
    uint64_t bh = H_INIT, bk = 0;
    for (uint64_t i = threadIdx.x; i < n_parts; i += blockDim.x) {
        const uint64_t h = part_h[i * stride + t], key = part_k[i * stride + t];
        if (h < bh || (h == bh && h != H_INIT && key < bk)) { bh = h; bk = key; }
    }
    sh[threadIdx.x] = bh;
    sk[threadIdx.x] = bk;
    __syncthreads();
    for (int d = 128; d >= 1; d >>= 1) {
        if ((int) threadIdx.x < d) {
            const uint64_t h = sh[threadIdx.x + d], key = sk[threadIdx.x + d];
            if (h < sh[threadIdx.x] || (h == sh[threadIdx.x] && h != H_INIT && key < sk[threadIdx.x])) {
                sh[threadIdx.x] = h;
                sk[threadIdx.x] = key;
            }
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        if (part_out) {
            part_out[t] = sh[0];
            part_out[m + t] = sk[0];
            return;
        }
        const uint64_t v = sh[0] == H_INIT ? 0ull : sk[0];
        if (sig_bytes == 4) reinterpret_cast<uint32_t *>(sig_out)[t] = (uint32_t) v;
        else reinterpret_cast<uint64_t *>(sig_out)[t] = v;
    }
}

// the forms the host side launches (kmu_sketch_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__(SketchArgs);
KMU_PMH_POINTS_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

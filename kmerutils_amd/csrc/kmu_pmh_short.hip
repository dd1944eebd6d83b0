// kmu_pmh_short.hip -- reads of at most 256 k-mers, one wave per read end to end: k_multiset_short, k_pmh_points_short.
#include "kmu_pmh_steps.h"

namespace kmu {

// ---- reads of at most 256 k-mers (short-read sequencers): the multiset by ONE WAVE per read ---------------------------------
// A 150 bp read has ~130 k-mers: a 512-thread workgroup of k_multiset_uq spends ten barriers on a quarter of a key per thread
// (12.9 ms for a million such reads).  Here a wave takes a read by itself: the lanes stage the read's <= 20 code words in the
// wave's corner of LDS, every lane makes up to four keys, and equal keys meet in a 512-slot open-addressing table of the wave
// (`ds_cmpst_rtn_b64` claims a slot, `ds_add` counts) -- exact, no barrier, 20 waves per CU.  The occupied slots leave as the
// (key, weight) list k_pmh_points reads (its result does not depend on the order of a list).  The all-ones value that marks
// a free slot can be a key: such keys are counted in a register and listed at the end.
// Taken by launch_pmh3a when the longest read of the batch has at most SHORT_KEYS k-mers.
__global__ void __launch_bounds__(256) k_multiset_short(SketchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    uint64_t *tk = reinterpret_cast<uint64_t *>(smem + (size_t) wave * SHORT_WAVE_BYTES);
    uint32_t *tc = reinterpret_cast<uint32_t *>(tk + SHORT_SLOTS);
    uint32_t *words = tc + SHORT_SLOTS;
    const KmerCfg cfg = a.cfg;
    const int k = cfg.k;
    const bool fast64 = cfg.fhash == KMU_FHASH_CANON_INVHASH && cfg.kmer_type == KMU_KMER64BIT; // (see k_multiset_uq)
    for (uint32_t t = (uint32_t) lane; t < SHORT_SLOTS; t += 64u) { tk[t] = ~0ull; tc[t] = 0u; }
    const uint64_t off_first = uniform_u64(a.offsets[0]);
    const uint64_t total = a.total_bytes ? a.total_bytes : uniform_u64(a.offsets[a.n_seq]);
    uint32_t q_next = 0, q_end = 0, bad = 0; // lane 0's cursor into the queue (wave_take)
    for (;;) {
        const uint32_t r = wave_take(a.queue, q_next, q_end, lane);
        if (r >= a.n_seq) break;
        SeqView sv;
        sv.base = a.bases; sv.packed = 0; sv.total = total;
        sv.begin = uniform_u64(a.offsets[r]);
        sv.len = uniform_u64(a.offsets[r + 1]) - sv.begin;
        const uint32_t L = sv.len >= 0x80000000ull ? 0xFFFFFFFFu : (uint32_t) sv.len;
        const uint32_t nk = L >= (uint32_t) k ? L - (uint32_t) k + 1u : 0u;
        if (L == 0 && lane == 0) atomicOr(a.err, DERR_EMPTY_SEQ);
        if (nk == 0) { // no k-mer: k_pmh_points writes the row of an empty multiset
            bad |= wave_validate_seq(sv, 0, 1, false);
            if (lane == 0) a.lst_n[r] = 0u;
            continue;
        }
        if (nk > SHORT_KEYS) { // (the host only sends batches whose longest read fits)
            if (lane == 0) { a.lst_n[r] = 0u; atomicOr(a.err, DERR_TABLE_FULL); }
            continue;
        }
        const uint32_t lead = seq_lead(sv), wfirst = lead >> 4;
        const uint32_t nw = (uint32_t) ((L - 1 + lead) >> 4) + 2; // the k-mers' windows + 1 (<= 20 words)
        if ((uint32_t) lane < nw) {
            uint32_t b;
            words[lane] = load_code_word(sv, (uint64_t) wfirst + (uint32_t) lane, b);
            bad |= b;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); // the wave's own LDS traffic is in order; this keeps the compiler from moving it
        __builtin_amdgcn_wave_barrier();
        uint32_t n_free_key = 0; // occurrences of the key that looks like a free slot (wave-uniform)
#pragma unroll
        for (int j = 0; j < (int) (SHORT_KEYS / 64); j++) {
            if (64u * (uint32_t) j >= nk) break; // (uniform: no lane has a k-mer in this slot or a later one)
            const uint32_t p = (uint32_t) lane + 64u * (uint32_t) j;
            const bool have = p < nk;
            uint64_t key = 0;
            if (have) {
                const uint64_t val = staged_kmer(words, p + lead - 16u * wfirst, k);
                const uint64_t rc = revcomp_val(val, k);
                key = fast64 ? int64_hash(rc < val ? rc : val) : apply_fhash(cfg, val, rc);
            }
            const bool odd = have && key == ~0ull;
            n_free_key += (uint32_t) __popcll(__ballot(odd));
            if (have && !odd) {
                uint32_t slot = mix32(key) & (SHORT_SLOTS - 1);
                for (;;) { // (256 keys at most in 512 slots: a free slot always turns up)
                    const uint64_t old = atomicCAS((unsigned long long *) &tk[slot], ~0ull, (unsigned long long) key);
                    if (old == ~0ull || old == key) { atomicAdd(&tc[slot], 1u); break; }
                    slot = (slot + 1) & (SHORT_SLOTS - 1);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        // ---- the occupied slots leave as the read's list (and the table is free again) ----
        const uint64_t lb = sv.begin - off_first;
        uint32_t n_out = 0;
#pragma unroll
        for (int s8 = 0; s8 < (int) (SHORT_SLOTS / 64); s8++) {
            const uint32_t slot = (uint32_t) s8 * 64u + (uint32_t) lane;
            const uint64_t kq = tk[slot];
            const bool occ = kq != ~0ull;
            const uint64_t om = __ballot(occ);
            if (occ) {
                const uint64_t at = lb + n_out + (uint32_t) __popcll(om & ((1ull << lane) - 1ull));
                a.lst_keys[at] = kq;
                a.lst_w[at] = tc[slot];
                tk[slot] = ~0ull;
                tc[slot] = 0u;
            }
            n_out += (uint32_t) __popcll(om);
        }
        if (n_free_key) {
            if (lane == 0) { a.lst_keys[lb + n_out] = ~0ull; a.lst_w[lb + n_out] = n_free_key; }
            n_out++;
        }
        if (lane == 0) a.lst_n[r] = n_out;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
    }
    if (bad) atomicOr(a.err, DERR_NON_ACGT);
}

// ---- the points of a SHORT list (at most 256 pairs: the reads k_multiset_short takes) ------------------------------------------
// A read with fewer keys than m ln m cannot prune: ~m H_m points (1 200 at m = 200) are drawn before every slot is hit, round
// after round over all keys.  k_pmh_points walks a list chunk by chunk, each chunk through all of ITS rounds with the
// generator replayed from the seed, which for three chunks of a 130-key read is three times eighteen chunk-rounds; here the
// wave keeps its <= 4 pairs per lane AND their generator states in registers and takes all keys through round i before
// round i + 1 (nine rounds for the same read), q_max refreshed once per round.  Same draws per key in the same order, same
// slot arithmetic: the rows are those of k_pmh_points (the result of ProbMinHash3a does not depend on the order of the keys).
template <bool SIG32>
__global__ void __launch_bounds__(256) k_pmh_points_short(SketchArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const int wave = threadIdx.x >> 6, lane = lane_id();
    constexpr bool sig32 = SIG32;
    uint64_t *hmin = reinterpret_cast<uint64_t *>(smem) + (size_t) wave * (2 * (size_t) a.m + 2);
    uint64_t *sig = hmin + a.m;
    double *winv_lut = reinterpret_cast<double *>(reinterpret_cast<uint64_t *>(smem) + (size_t) 4 * (2 * (size_t) a.m + 2));
    for (uint32_t t = threadIdx.x; t < WINV_LUT; t += blockDim.x) winv_lut[t] = winv_entry(t);
    __syncthreads();
    constexpr int NJ = (int) (SHORT_KEYS / 64);
    // lane 0: reads are taken QCHUNK at a time -- wave_take (kmu_pmh_steps.h) spelled out: through the function this kernel came out two
    // instructions longer and outside the spread of two runs of the code before on the short-read workload (the split's table)
    uint32_t q_next = 0, q_end = 0;
    for (;;) {
        uint32_t r = 0;
        if (lane == 0) {
            if (q_next == q_end) {
                q_next = atomicAdd(a.queue2, (uint32_t) QCHUNK);
                q_end = q_next + QCHUNK;
            }
            r = q_next++;
        }
        r = uniform_u32(r);
        if (r >= a.n_seq) break;
        const uint64_t base = a.offsets[r] - a.offsets[0];
        const uint32_t n = a.lst_n[r]; // <= SHORT_KEYS + 1 (the all-ones key, if any, sits behind the table's pairs)
        uint64_t key[NJ + 1];
        double winv[NJ + 1];
        Xoshiro rng[NJ + 1];
        bool alive[NJ + 1];
#pragma unroll
        for (int j = 0; j <= NJ; j++) {
            const uint32_t i = (uint32_t) lane + 64u * (uint32_t) j;
            alive[j] = false;
            key[j] = 0;
            winv[j] = 0.0;
            if (i < n && (j < NJ || lane == 0)) {
                key[j] = a.lst_keys[base + i];
                const uint32_t w = a.lst_w[base + i];
                winv[j] = winv_of(winv_lut, w);
                alive[j] = w != 0u;
            }
        }
        for (int t = lane; t < a.m; t += 64) { hmin[t] = H_INIT; sig[t] = 0; }
        uint64_t qb = H_INIT;
        // ---- round 1: the first point of every key (pmh3a_first_point, with the generator kept) ----
#pragma unroll
        for (int j = 0; j <= NJ; j++) {
            if (__any(alive[j])) {
                if (alive[j]) {
                    rng[j].seed(hasher_finish(KMU_HASHER_NOHASH, key[j], sig32));
                    const double x = exp01_sample(a.e01, rng[j]);
                    const double h = winv[j] * x, qmax = __longlong_as_double((long long) qb);
                    if (h < qmax) {
                        const uint32_t k = draw_slot(a, rng[j]);
                        slot_update_wave(hmin, sig, k, h, key[j]);
                        alive[j] = winv[j] < qmax; // the crate: `if winv < qmax { to_be_processed.push(..) }`
                    } else {
                        alive[j] = false;
                    }
                }
                qb = wave_qmax(hmin, a.m);
            }
        }
        // ---- rounds i >= 2, all keys through a round before the next (pmh3a_more_points without the replay) ----
        for (uint32_t i = 2;; i++) {
            bool any = false;
#pragma unroll
            for (int j = 0; j <= NJ; j++) {
                if (__any(alive[j])) {
                    any = true;
                    if (alive[j]) {
                        const double qmax = __longlong_as_double((long long) qb);
                        const double hbase = winv[j] * (double) (i - 1);
                        if (!(hbase < qmax)) {
                            alive[j] = false;
                        } else {
                            const double x = exp01_sample(a.e01, rng[j]);
                            const double h = hbase + winv[j] * x;
                            const uint32_t k = draw_slot(a, rng[j]); // rounds >= 2 always draw the slot
                            if (h < qmax) slot_update_wave(hmin, sig, k, h, key[j]);
                            if (!(winv[j] * (double) i < qmax)) alive[j] = false;
                        }
                    }
                }
            }
            if (!any) break;
            qb = wave_qmax(hmin, a.m);
        }
        // ---- signature row: arg-min key per slot, initobj (0) for an empty multiset ----
        for (int t = lane; t < a.m; t += 64) {
            const uint64_t v = hmin[t] == H_INIT ? 0ull : sig[t];
            if (sig32) reinterpret_cast<uint32_t *>(a.sig_out)[(uint64_t) r * a.m + t] = (uint32_t) v;
            else reinterpret_cast<uint64_t *>(a.sig_out)[(uint64_t) r * a.m + t] = v;
        }
    }
}

// the forms the host side launches (kmu_sketch_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__(SketchArgs);
KMU_PMH_SHORT_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

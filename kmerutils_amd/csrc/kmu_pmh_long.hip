// kmu_pmh_long.hip -- k_multiset_long: the multiset of a read too long for the registers of one workgroup, as hash-partitioned sub-lists
// that each go through k_multiset_uq's step (occupancy bitmaps, keys that occur once straight to the list, the others merged by a miniature sort).
#include "kmu_pmh_steps.h"
#include "kmu_sketch_host.hpp"

namespace kmu {

// ---- reads of more than UQ_KEYS places: sub-lists by key hash, the uq step on each ------------------------------------------
// The general list-emitting kernel ranks, scans, places and searches EVERY key of such a read in its 4 096-bucket counting sort, in at
// least three hash partitions whose later keys are parked in HBM and ranked again.  Here a read is scanned once (phase A): every
// key is appended to one of P = pmh_long_parts(nk) sub-lists in the workgroup's own scratch, chosen by pmh_long_part_of -- hash bits
// that are independent of the bitmap index and of the collision sort's bucket.  Equal keys share a sub-list, so a sub-list is a
// multiset of its own and nothing is ever merged across sub-lists.  Phase B takes the sub-lists in turn, 20 keys per thread as in
// k_multiset_uq<1024, ...>: bitmap A / B, one barrier, B clear = weight 1 = list entry at the read's running unique cursor; B set =
// collected, merged by the 1 024-thread miniature sort, and set aside (key, weight) behind the sub-list in scratch, because the
// entries with a weight stand BEHIND all unique ones in the read's list and the unique count is known only after the last
// sub-list.  They are copied there at the end of the read's turn.  Output: the lists k_pmh_points reads, as k_multiset_uq writes them.
// A read falls back to the general kernel (redo_list, lst_n = lst_nu = 0) when a sub-list outgrows a workgroup's registers, a
// sub-list collects more than UQ2_COLL keys, or P > DEF_PARTS; so does a read of at most UQ_KEYS places, which is on this
// kernel's list only because the second uq shape found it too repetitive.
// Scratch (a.def_keys, [grid][DEF_PARTS][DEF_SEG] keys): segment p = sub-list p in [0, UQ_KEYS), its collected keys in
// [UQ_KEYS, UQ_KEYS + UQ2_COLL), their weights (32 bits each) behind them.  It is re-used read after read by the same CU: every
// store and load of it is the agent-scope form of the general kernel (a plain load can hit a stale line of this CU's L1), with
// a workgroup barrier that waits for the stores between the phases.
template <typename T>
__device__ __forceinline__ T ld_scr(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
template <typename T>
__device__ __forceinline__ void st_scr(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ void __launch_bounds__(1024, 4) k_multiset_long(SketchArgs a) {
    constexpr int UQ_THREADS = 1024;
    constexpr uint32_t UQ_BM_BITS = UQ2_BM, UQ_COLL = UQ2_COLL;
    typedef UqShape<UQ_THREADS, UQ_BM_BITS, UQ_COLL> SH;
    constexpr uint32_t UQ_KEYS = SH::KEYS, UQ_BM_WORDS = SH::BM_WORDS, UQ_BUCKETS = SH::BUCKETS, UQ_TILE = SH::TILE;
    constexpr uint32_t TILE_WORDS = UQ_KEYS / 16; // code words whose k-mers one tile of phase A takes (two more are staged behind them)
    static_assert((UQ_BM_WORDS / 4) % (uint32_t) UQ_THREADS == 0, "whole 16-byte stores per thread wipe a bitmap");
    static_assert(UQ_COLL % UQ_THREADS == 0 && UQ_COLL / UQ_THREADS <= 4, "collected keys per thread");
    static_assert(TILE_WORDS + 2 <= UQ_TILE, "a tile's words and the two behind them fit the staged words");
    static_assert(UQ_KEYS + UQ_COLL + UQ_COLL / 2 <= DEF_SEG, "a segment holds a sub-list, its collected keys and their weights");
    static_assert(PMH_LONG_TP < UQ_KEYS, "a sub-list of the expected size fits the registers");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *bmA = reinterpret_cast<uint32_t *>(smem);
    uint32_t *bmB = bmA + UQ_BM_WORDS;
    uint64_t *ck = reinterpret_cast<uint64_t *>(bmB + UQ_BM_WORDS); // keys of the collision groups, as collected
    uint64_t *dk = ck + UQ_COLL;                                     // ... grouped by bucket
    uint32_t *dw = reinterpret_cast<uint32_t *>(dk + UQ_COLL);
    uint32_t *bst = dw + UQ_COLL;          // UQ_BUCKETS + 1
    uint32_t *words = bst + UQ_BUCKETS + 1; // UQ_TILE
    uint32_t *wtot = words + UQ_TILE;       // one per wave
    // [0] unique entries of the read so far, [1] keys in collision groups of the sub-list in hand, [4] the read in hand, [5] the next,
    // [8 .. 11] thread 0's cursor into the read queue (as in k_multiset_uq)
    uint32_t *misc = wtot + UQ_THREADS / 64;
    // (the landing area of k_multiset_uq's prefetched chunks is free here: the words of a tile are staged by plain loads)
    constexpr uint32_t RAW_OFF = ((8u * UQ_BM_WORDS + 20u * UQ_COLL + 4u * (UQ_BUCKETS + 1u + UQ_TILE + (uint32_t) UQ_THREADS / 64u) + 64u) + 15u) & ~15u;
    static_assert(RAW_OFF + 8u * DEF_PARTS <= SH::LDS, "the sub-lists' counters lie inside the shape's LDS");
    uint32_t *pcnt = reinterpret_cast<uint32_t *>(smem + RAW_OFF); // keys of sub-list p
    uint32_t *ccnt = pcnt + DEF_PARTS;                              // ... its (key, weight) entries set aside
    const KmerCfg cfg = a.cfg;
    const int k = cfg.k, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    uint64_t *seg0 = a.def_keys + (uint64_t) blockIdx.x * DEF_CAP;
    for (uint32_t i = tid; i < UQ_BUCKETS + 1; i += UQ_THREADS) bst[i] = 0;
    auto take = [&]() -> uint32_t { // thread 0: the next queue entry (the queue is asked a read before the chunk runs out)
        if (misc[8] == misc[9]) {
            if (!misc[11]) misc[10] = atomicAdd(KMU_COLD_ARG(queue), (uint32_t) QCHUNK);
            misc[8] = misc[10];
            misc[9] = misc[10] + QCHUNK;
            misc[11] = 0;
        }
        const uint32_t v = misc[8]++;
        if (misc[8] == misc[9] && !misc[11]) { misc[10] = atomicAdd(KMU_COLD_ARG(queue), (uint32_t) QCHUNK); misc[11] = 1; }
        return v;
    };
    if (tid == 0) {
        misc[8] = misc[9] = misc[10] = misc[11] = 0;
        misc[4] = take();
    }
    __syncthreads();
    const uint64_t off_first = uniform_u64(a.offsets[0]);
    const uint64_t total = a.total_bytes ? a.total_bytes : uniform_u64(a.offsets[a.n_seq]);
    auto seq_of = [&](uint32_t q) -> uint32_t {
        const uint32_t *rl = KMU_COLD_ARG(read_list);
        return rl ? rl[q] : q;
    };
    uint32_t r = uniform_u32(misc[4]);
    uint32_t rs = r < a.n_queue ? uniform_u32(seq_of(r)) : 0u; // the sequence
    SeqView sv;
    sv.base = a.bases; sv.packed = 0; sv.total = total; sv.begin = 0; sv.len = 0;
    if (r < a.n_queue) { sv.begin = uniform_u64(a.offsets[rs]); sv.len = uniform_u64(a.offsets[rs + 1]) - sv.begin; }
    auto place_of = [&](int q) -> uint32_t { return 4u * ((uint32_t) tid + (uint32_t) UQ_THREADS * (uint32_t) (q >> 2)) + (uint32_t) (q & 3); };
    auto bm_index = [&](uint64_t key) -> uint32_t { // (k_multiset_uq's)
        return (((uint32_t) key ^ (uint32_t) (key >> 32)) * 0x85EBCA6Bu) >> (32 - UQ_BM_BITS);
    };
    while (r < a.n_queue) {
        if (tid == 0) {
            misc[5] = take(); // the read after this one
            misc[0] = 0;
        }
        if (tid < (int) DEF_PARTS) pcnt[tid] = 0;
        const uint32_t L = sv.len >= 0x80000000ull ? 0xFFFFFFFFu : (uint32_t) sv.len;
        const uint32_t nk = L >= (uint32_t) k ? L - (uint32_t) k + 1u : 0u;
        const uint32_t lead = seq_lead(sv), wfirst = lead >> 4, l0 = lead - 16u * wfirst; // l0: place of the read's first base
        const uint32_t span = uniform_u32(nk + l0); // places: the read's k-mers behind the lead of its first word
        const uint32_t P = uniform_u32(pmh_long_parts(nk));
        const bool mine = nk >= 1u && L != 0xFFFFFFFFu && span > UQ_KEYS && P <= DEF_PARTS;
        uint32_t bad = 0;
        lds_barrier();
        const uint32_t r_next = uniform_u32(misc[5]);
        const bool has_next = r_next < a.n_queue;
        // the header of the next read: requested now, looked at at the end of this turn
        const uint32_t rs_n = has_next ? seq_of(r_next) : 0u;
        const uint64_t n_o0 = has_next ? a.offsets[rs_n] : 0ull, n_o1 = has_next ? a.offsets[rs_n + 1] : 0ull;
        bool over = false; // uniform: a sub-list too long for the registers, or too many keys in its collision groups
        uint32_t n_u = 0, n_ct = 0;
        if (mine) {
            // ---- phase A: the read tile by tile; every key to its sub-list (one ds_add_rtn per key at the sub-list's counter, as the
            // general kernel parks its later partitions' keys: three instructions per key where a ballot per sub-list and wave takes 4 P)
            const uint32_t nw_all = (uint32_t) ((L - 1 + lead) >> 4) + 2; // staged words of the whole read (its k-mers' windows + 1)
            auto scan_phase = [&](auto fast_tag) __attribute__((always_inline)) {
                constexpr bool FAST = decltype(fast_tag)::value;
                for (uint32_t t0 = 0; t0 < span; t0 += UQ_KEYS) { // t0: first place of the tile
                    const uint32_t w0 = t0 >> 4;
                    const uint32_t nwt = nw_all - w0 < TILE_WORDS + 2 ? nw_all - w0 : TILE_WORDS + 2;
                    for (uint32_t t = tid; t < nwt; t += UQ_THREADS) {
                        uint32_t b;
                        words[t] = load_code_word(sv, (uint64_t) wfirst + w0 + t, b);
                        bad |= b;
                    }
                    lds_barrier();
                    const uint32_t span_t = span - t0; // places of this tile and the ones behind it
                    const int kq = (int) opaque_u32((uint32_t) k); // (the k-mer mask and shift: formed here, as in k_multiset_uq)
#pragma unroll
                    for (int q0 = 0; q0 < UQ_KREG; q0 += 4) {
                        if (!(4u * (uint32_t) UQ_THREADS * (uint32_t) (q0 >> 2) < span_t)) continue;
                        const uint32_t wi = ((uint32_t) tid >> 2) + (uint32_t) (UQ_THREADS / 4) * (uint32_t) (q0 >> 2); // the quarter's word
                        const StepWin sw = step_win(words[wi], words[wi + 1], words[wi + 2], kq);
                        // the four keys of the quarter first, then their four ds_add_rtn, then the answers: no answer is looked at inside the
                        // per-lane branch that asked for it (where it was waited for on the spot: one LDS round trip per key, in turn)
                        uint64_t key[4];
                        uint32_t part[4], at[4];
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            key[u] = 0;
                            part[u] = 0xFFFFFFFFu; // no key
                            if (t0 + place_of(q0 + u) - l0 < nk) {
                                uint64_t val, rc;
                                step_val_rc_lane(sw, 4u * ((uint32_t) tid & 3u) + (uint32_t) u, val, rc);
                                key[u] = FAST ? int64_hash(rc < val ? rc : val) : apply_fhash(cfg, val, rc);
                                part[u] = pmh_long_part_of(key[u], P);
                            }
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++) {
                            at[u] = 0xFFFFFFFFu;
                            if (part[u] != 0xFFFFFFFFu) at[u] = atomicAdd(&pcnt[part[u]], 1u);
                        }
#pragma unroll
                        for (int u = 0; u < 4; u++)
                            if (at[u] < UQ_KEYS) st_scr(&seg0[(uint64_t) part[u] * DEF_SEG + at[u]], key[u]);
                    }
                    lds_barrier(); // (the next tile's words replace these)
                }
            };
            if (cfg.fhash == KMU_FHASH_CANON_INVHASH && cfg.kmer_type == KMU_KMER64BIT) scan_phase(std::true_type{});
            else scan_phase(std::false_type{});
            __syncthreads(); // every key of the read is in its sub-list (the stores have completed: vmcnt(0))
            // ---- phase B: the sub-lists in turn through the uq step ----
            const uint64_t lb = sv.begin - off_first; // list entries of read r start here
            for (uint32_t p = 0; p < P && !over; p++) {
                const uint32_t n_p = uniform_u32(pcnt[p]);
                if (n_p > UQ_KEYS) { over = true; break; }
                uint64_t *seg = seg0 + (uint64_t) p * DEF_SEG;
                uint4 *za = reinterpret_cast<uint4 *>(bmA), *zb = reinterpret_cast<uint4 *>(bmB);
#pragma unroll
                for (uint32_t z = 0; z < UQ_BM_WORDS / 4 / (uint32_t) UQ_THREADS; z++) {
                    za[tid + z * UQ_THREADS] = make_uint4(0u, 0u, 0u, 0u);
                    zb[tid + z * UQ_THREADS] = make_uint4(0u, 0u, 0u, 0u);
                }
                if (tid == 0) misc[1] = 0;
                lds_barrier();
                // Register slots 4 g .. 4 g + 3 of all threads stand for entries [4 UQ_THREADS g, 4 UQ_THREADS (g + 1)) of the sub-list: slot q
                // of thread t is entry q UQ_THREADS + t.  A group the sub-list does not reach issues nothing, in both phases, by one test.
                auto group_used = [&](int q0) -> bool { return 4u * (uint32_t) UQ_THREADS * (uint32_t) (q0 >> 2) < n_p; };
                uint64_t rk[UQ_KREG];
#pragma unroll
                for (int q0 = 0; q0 < UQ_KREG; q0 += 4) {
                    if (!group_used(q0)) {
                        // (no instruction: the slots are told to hold nothing in particular, or they carry the last sub-list's keys around the loops)
#pragma unroll
                        for (int u = 0; u < 4; u++) rk[q0 + u] = __builtin_nondeterministic_value(rk[q0 + u]);
                        continue;
                    }
                    uint32_t bit[4], rbw[4], rbb[4]; // a slot's word of the bitmap and its bit there
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t e = (uint32_t) (q0 + u) * UQ_THREADS + (uint32_t) tid;
                        rk[q0 + u] = 0;
                        if (e < n_p) rk[q0 + u] = ld_scr(&seg[e]);
                    }
                    // (as in k_multiset_uq: a slot without a key ORs nothing into its thread's own word, the four ds_or_rtn leave back
                    //  to back outside every per-lane branch and are looked at together)
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint32_t e = (uint32_t) (q0 + u) * UQ_THREADS + (uint32_t) tid;
                        const uint32_t bi = bm_index(rk[q0 + u]);
                        rbw[u] = e < n_p ? bi >> 5 : (uint32_t) tid;
                        rbb[u] = e < n_p ? 1u << (bi & 31u) : 0u;
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) bit[u] = atomicOr(&bmA[rbw[u]], rbb[u]);
#pragma unroll
                    for (int u = 0; u < 4; u++) bit[u] &= rbb[u];
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (bit[u]) atomicOr(&bmB[rbw[u]], bit[u]);
                }
                lds_barrier();
                // ---- sort out: B bit clear = occurs once = list entry (key, 1) from the register; else collect ----
#pragma unroll
                for (int q0 = 0; q0 < UQ_KREG; q0 += 4) {
                    if (!group_used(q0)) continue; // (its rk[] hold no key)
                    bool uq[4], co[4];
                    uint64_t um[4], cm[4];
                    uint32_t ut = 0, ct = 0, bw[4];
                    // (the four B words are read by every lane -- a slot without a key holds key 0 -- and looked at together)
#pragma unroll
                    for (int u = 0; u < 4; u++) bw[u] = bmB[bm_index(rk[q0 + u]) >> 5];
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const bool have = (uint32_t) (q0 + u) * UQ_THREADS + (uint32_t) tid < n_p;
                        co[u] = have && (bw[u] & (1u << (bm_index(rk[q0 + u]) & 31u))) != 0u;
                        uq[u] = have && !co[u];
                    }
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        um[u] = __ballot(uq[u]);
                        cm[u] = __ballot(co[u]);
                        ut += (uint32_t) __popcll(um[u]);
                        ct += (uint32_t) __popcll(cm[u]);
                    }
                    uint32_t ub = 0, cb = 0; // one atomic per wave, list and group of four register slots
                    // (lane 0 by a compare made here, the counters addressed from the lane: see opaque_lane_u32)
                    const uint32_t ln = opaque_lane_u32((uint32_t) lane), z0 = opaque_lane_u32(0u);
                    if (ln == 0) {
                        if (ut) ub = atomicAdd(lane_ptr(misc, z0), ut);
                        if (ct) cb = atomicAdd(lane_ptr(misc + 1, z0), ct);
                    }
                    ub = bcast_u32(ub, 0);
                    cb = bcast_u32(cb, 0);
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const uint64_t below = (1ull << lane) - 1ull;
                        if (uq[u]) {
                            const uint64_t at = lb + ub + (uint32_t) __popcll(um[u] & below);
                            a.lst_keys[at] = rk[q0 + u]; // (weight 1, implied: lst_nu)
                        }
                        if (co[u]) {
                            const uint32_t at = cb + (uint32_t) __popcll(cm[u] & below);
                            if (at < UQ_COLL) ck[at] = rk[q0 + u];
                        }
                        ub += (uint32_t) __popcll(um[u]);
                        cb += (uint32_t) __popcll(cm[u]);
                    }
                }
                lds_barrier();
                const uint32_t n_c = uniform_u32(misc[1]);
                if (n_c > UQ_COLL) { over = true; break; }
                if (tid == 0) ccnt[p] = n_c;
                if (n_c) {
                    // ---- the collision groups: counting sort on 11 hash bits, equal keys hand their weight to the first ----
                    uint64_t key[UQ_COLL / UQ_THREADS];
                    uint32_t rb[UQ_COLL / UQ_THREADS];
#pragma unroll
                    for (int j = 0; j < (int) (UQ_COLL / UQ_THREADS); j++) {
                        const uint32_t i = (uint32_t) j * UQ_THREADS + tid;
                        rb[j] = 0xFFFFFFFFu;
                        key[j] = 0;
                        if (i < n_c) {
                            key[j] = ck[i];
                            const uint32_t b = mix32(key[j]) / (0x80000000u / (UQ_BUCKETS / 2)); // the top log2(UQ_BUCKETS) bits
                            rb[j] = (b << 16) | atomicAdd(&bst[b], 1u);
                        }
                    }
                    lds_barrier();
                    { // exclusive scan of the bucket counts, two per thread
                        const uint32_t c0 = bst[2 * tid], c1 = bst[2 * tid + 1];
                        const uint32_t incl = wave_incl_scan_u32(c0 + c1);
                        if (lane == 63) wtot[wave] = incl;
                        lds_barrier();
                        uint32_t pre = incl - (c0 + c1);
#pragma unroll
                        for (int w = 0; w < UQ_THREADS / 64; w++) pre += w < wave ? wtot[w] : 0u;
                        bst[2 * tid] = pre;
                        bst[2 * tid + 1] = pre + c0;
                    }
                    lds_barrier();
#pragma unroll
                    for (int j = 0; j < (int) (UQ_COLL / UQ_THREADS); j++)
                        if (rb[j] != 0xFFFFFFFFu) {
                            const uint32_t pos = bst[rb[j] >> 16] + (rb[j] & 0xFFFFu);
                            rb[j] = (rb[j] & 0xFFFF0000u) | pos;
                            dk[pos] = key[j];
                            dw[pos] = 1u;
                        }
                    lds_barrier();
#pragma unroll
                    for (int j = 0; j < (int) (UQ_COLL / UQ_THREADS); j++)
                        if (rb[j] != 0xFFFFFFFFu) {
                            const uint32_t pos = rb[j] & 0xFFFFu;
                            for (uint32_t t = bst[rb[j] >> 16]; t < pos; t++)
                                if (dk[t] == key[j]) { // the first equal key of the bucket takes this one's weight
                                    dw[pos] = 0u;
                                    atomicAdd(&dw[t], 1u);
                                    break;
                                }
                        }
                    lds_barrier();
                    // set aside behind the sub-list: the entries' place in the read's list is known after the last sub-list
                    uint32_t *seg_w = reinterpret_cast<uint32_t *>(seg + UQ_KEYS + UQ_COLL);
                    for (uint32_t i = tid; i < n_c; i += UQ_THREADS) {
                        st_scr(&seg[UQ_KEYS + i], dk[i]);
                        st_scr(&seg_w[i], dw[i]);
                    }
                    bst[2 * tid] = 0;
                    bst[2 * tid + 1] = 0;
                }
                lds_barrier();
            }
            __syncthreads(); // (the entries set aside have reached memory; ccnt[] is written)
            if (!over) {
                n_u = uniform_u32(misc[0]);
                uint32_t *lst_w = KMU_COLD_ARG(lst_w);
                for (uint32_t p = 0; p < P; p++) {
                    const uint32_t n_c = uniform_u32(ccnt[p]);
                    const uint64_t *seg = seg0 + (uint64_t) p * DEF_SEG;
                    const uint32_t *seg_w = reinterpret_cast<const uint32_t *>(seg + UQ_KEYS + UQ_COLL);
                    for (uint32_t i = tid; i < n_c; i += UQ_THREADS) {
                        a.lst_keys[lb + n_u + n_ct + i] = ld_scr(&seg[UQ_KEYS + i]);
                        lst_w[lb + n_u + n_ct + i] = ld_scr(&seg_w[i]);
                    }
                    n_ct += n_c;
                }
            }
        }
        if (tid == 0) {
            if (mine && !over) { KMU_COLD_ARG(lst_n)[rs] = n_u + n_ct; KMU_COLD_ARG(lst_nu)[rs] = n_u; }
            else if (nk != 0) { // the general kernel's
                KMU_COLD_ARG(lst_n)[rs] = 0u;
                KMU_COLD_ARG(lst_nu)[rs] = 0u;
                KMU_COLD_ARG(redo_list)[atomicAdd(KMU_COLD_ARG(queue) + 56, 1u)] = rs;
            }
        }
        if (bad) atomicOr(KMU_COLD_ARG(err), DERR_NON_ACGT);
        r = r_next;
        rs = uniform_u32(rs_n);
        if (has_next) {
            sv.begin = uniform_u64(n_o0);
            sv.len = uniform_u64(n_o1) - sv.begin;
        }
        lds_barrier();
    }
}

} // namespace kmu

// kmu_pmh_uq.hip -- k_multiset_uq: the multiset of a read that fits the registers of one workgroup, without sorting what occurs once.
#include "kmu_pmh_steps.h"

namespace kmu {

// ---- reads that fit the registers of one workgroup: the multiset without a counting sort ------------------------------------
// In a noisy long read almost every 31-mer occurs once.  k_multiset_uq does not sort what does not need sorting: every key
// sets its bit in an occupancy bitmap A of 2^16 bits (a second hash of the key; `ds_or_rtn`), a key that finds its bit set also
// sets it in B.  After one barrier a key whose B bit is clear has PROVABLY met no equal key -- weight 1, final -- and leaves
// for the (key, weight) lists straight from the registers (nine keys in ten of an ONT read at k = 31).  The others, a few
// hundred per read, are collected in LDS and merged exactly by a miniature of the general kernel's counting sort (1 024
// buckets, rank / scan / place / walk).  No partitions, blocks, rounds, parked keys: the kernel is small, a workgroup is 512
// threads with 20 keys per thread, and TWO workgroups share a CU, so one read's barriers hide under the other's work.
// Reads with more than UQ_KEYS k-mers (or more than UQ_COLL keys in collision groups) are appended to `redo_list` and taken
// by the general list-emitting kernel in a second launch.  Output: the lists k_pmh_points reads, as k_sketch_pmh3a<EMIT>.
// Two shapes: <512 threads, 2^17-bit bitmaps, 1 024 collected keys> for reads of up to 10 240 k-mers, two workgroups per CU;
// <1024, 2^18, 2 048> for up to 20 480 k-mers, one workgroup per CU, run on the list the first shape leaves behind.
// every vector-memory request of this wave has completed (the chunks of global_load_lds have landed in LDS)
__device__ __forceinline__ void vm_wait_lds_loads() {
    __builtin_amdgcn_s_waitcnt(0x0F70); // vmcnt(0); expcnt / lgkmcnt untouched
    asm volatile("" ::: "memory");
}
// (Round 4, measured and not kept: the collision groups through an open-addressing table in LDS instead of the counting sort --
// 10.13 against 10.10 ms per launch: with two workgroups per CU the barriers of one hide under the other's key phase.)

template <int UQ_THREADS, uint32_t UQ_BM_BITS, uint32_t UQ_COLL, int MINW>
__global__ void __launch_bounds__(UQ_THREADS, MINW) k_multiset_uq(SketchArgs a) {
    typedef UqShape<UQ_THREADS, UQ_BM_BITS, UQ_COLL> SH;
    constexpr uint32_t UQ_KEYS = SH::KEYS, UQ_BM_WORDS = SH::BM_WORDS, UQ_BUCKETS = SH::BUCKETS, UQ_TILE = SH::TILE;
    static_assert((UQ_BM_WORDS / 4) % (uint32_t) UQ_THREADS == 0, "whole 16-byte stores per thread wipe a bitmap");
    static_assert(UQ_COLL % UQ_THREADS == 0 && UQ_COLL / UQ_THREADS <= 4, "collected keys per thread");
    static_assert((uint32_t) UQ_THREADS <= UQ_BM_WORDS, "every thread has a word of bitmap A of its own");
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint32_t *bmA = reinterpret_cast<uint32_t *>(smem);
    uint32_t *bmB = bmA + UQ_BM_WORDS;
    uint64_t *ck = reinterpret_cast<uint64_t *>(bmB + UQ_BM_WORDS); // keys of the collision groups, as collected
    uint64_t *dk = ck + UQ_COLL;                                     // ... grouped by bucket
    uint32_t *dw = reinterpret_cast<uint32_t *>(dk + UQ_COLL);
    uint32_t *bst = dw + UQ_COLL;          // UQ_BUCKETS + 1
    uint32_t *words = bst + UQ_BUCKETS + 1; // UQ_TILE
    uint32_t *wtot = words + UQ_TILE;       // one per wave
    // [0] unique entries, [1] keys in collision groups, [4] first read, [5] the read after it, [6] the queue entry taken last (three reads ahead)
    uint32_t *misc = wtot + UQ_THREADS / 64;
    // the next read's chunks land here straight from HBM (global_load_lds: no register is held while they are in flight):
    // chunk t of the read at byte 16 t, i.e. lane l of the wave instruction that fetches chunks 64 j .. 64 j + 63 at 1024 j + 16 l
    // (its place as an offset from the 16-byte aligned base: a pointer that went through an integer is a FLAT pointer to the compiler --
    //  64-bit address arithmetic kept in registers the kernel does not have, spilled, and FLAT instead of LDS accesses)
    constexpr uint32_t RAW_OFF = ((8u * UQ_BM_WORDS + 20u * UQ_COLL + 4u * (UQ_BUCKETS + 1u + UQ_TILE + (uint32_t) UQ_THREADS / 64u) + 64u) + 15u) & ~15u;
    uint8_t *rawp = smem + RAW_OFF;
    const KmerCfg cfg = a.cfg;
    const int k = cfg.k, tid = threadIdx.x, lane = lane_id(), wave = tid >> 6;
    for (uint32_t i = tid; i < UQ_BUCKETS + 1; i += UQ_THREADS) bst[i] = 0;
    // thread 0's cursor into the read queue: misc[8] next, [9] end of the chunk in hand, [10] the chunk asked for ahead, [11] whether one
    // is (in LDS: registers of thread 0 alone would be registers of every thread)
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
        misc[5] = take(); // the header of a read is fetched TWO reads ahead: its words can then be requested a whole read ahead
        misc[6] = take(); // ... and its entry of read_list (the second shape's launch) THREE reads ahead: the header's address is then known
    }
    __syncthreads();
    const uint64_t off_first = uniform_u64(a.offsets[0]);
    const uint64_t total = a.total_bytes ? a.total_bytes : uniform_u64(a.offsets[a.n_seq]);
    // queue entry q stands for sequence read_list[q] when a list is given (the second shape's launch), else for sequence q
    auto seq_of = [&](uint32_t q) -> uint32_t {
        const uint32_t *rl = KMU_COLD_ARG(read_list);
        return rl ? rl[q] : q;
    };
    uint32_t r = uniform_u32(misc[4]);
    uint32_t rs = r < a.n_queue ? uniform_u32(seq_of(r)) : 0u; // the sequence
    SeqView sv;
    sv.base = a.bases; sv.packed = 0; sv.total = total; sv.begin = 0; sv.len = 0;
    if (r < a.n_queue) { sv.begin = uniform_u64(a.offsets[rs]); sv.len = uniform_u64(a.offsets[rs + 1]) - sv.begin; }
    // A thread's register slots stand for positions in the frame of the staged words (place = position + the place of the read's
    // first base in its first word, seq_lead): slots 4 i .. 4 i + 3 = the four places of quarter (tid + UQ_THREADS x i) of the
    // words.  The four k-mers of a quarter come out of ONE window of three words, their reverse complements out of the window's
    // reverse complement (StepWin: 12 instead of 26 instructions per k-mer for extraction and reverse complement, 0.75 instead
    // of 3 LDS reads; round 4 -- before, slot q was position q x UQ_THREADS + tid.  Whole words per thread -- constant shifts,
    // 7 instructions -- leave a quarter of the threads of a typical read without a k-mer: 13.3 against 11.7 ms per launch).
    auto fits = [&](const SeqView &v) -> bool { // a read this shape takes
        const uint32_t Lv = v.len >= 0x80000000ull ? 0xFFFFFFFFu : (uint32_t) v.len;
        return Lv >= (uint32_t) k && Lv - (uint32_t) k + 1u + seq_lead(v) <= UQ_KEYS;
    };
    static_assert(UQ_KREG % 4 == 0 && UQ_THREADS % 4 == 0, "quarters of words");
    auto place_of = [&](int q) -> uint32_t { return 4u * ((uint32_t) tid + (uint32_t) UQ_THREADS * (uint32_t) (q >> 2)) + (uint32_t) (q & 3); };
    // the read after the current one: header known from the start of the current read's turn
    uint32_t r_next = uniform_u32(misc[5]);
    uint32_t rs_next = r_next < a.n_queue ? uniform_u32(seq_of(r_next)) : 0u;
    SeqView nv = sv;
    bool nv_mine = false;
    if (r_next < a.n_queue) {
        nv.begin = uniform_u64(a.offsets[rs_next]);
        nv.len = uniform_u64(a.offsets[rs_next + 1]) - nv.begin;
        nv_mine = fits(nv);
    }
    // the read after next: its sequence is known from the start of the current read's turn (asked for a turn earlier, looked at at the end
    // of that turn: the list entry and the header it points to are a dependent pair of round trips, and every wave of the workgroup sat
    // out the first of them at the top of each turn)
    uint32_t r_nn = uniform_u32(misc[6]);
    uint32_t rs_nn = r_nn < a.n_queue ? uniform_u32(seq_of(r_nn)) : 0u;
    __syncthreads(); // (misc[6] is rewritten at the top of the first turn)
    uint32_t pf_bad = 0; // non-ACGT bytes among this thread's words of the current read, fetched a read ahead
    bool pf_valid = false;                    // uniform
    auto n_words = [&](const SeqView &v) -> uint32_t { // staged words of a read of 1 .. UQ_KEYS k-mers (its k-mers' windows + 1)
        const uint32_t Lv = (uint32_t) v.len, ld = seq_lead(v);
        return (uint32_t) ((Lv - 1 + ld) >> 4) + 2;
    };
    while (r < a.n_queue) {
        if (tid == 0) {
            misc[6] = take(); // the read three behind the current one
            misc[0] = 0;
            misc[1] = 0;
        }
        const uint32_t L = sv.len >= 0x80000000ull ? 0xFFFFFFFFu : (uint32_t) sv.len;
        const uint32_t nk = L >= (uint32_t) k ? L - (uint32_t) k + 1u : 0u;
        const bool mine = nk >= 1u && nk + seq_lead(sv) <= UQ_KEYS; // else: no k-mer at all (row of zeros), or the general kernel's
        uint32_t bad = 0;
        if (L == 0 && tid == 0) atomicOr(KMU_COLD_ARG(err), DERR_EMPTY_SEQ);
        if (nk == 0) bad |= wave_validate_seq(sv, wave, UQ_THREADS / 64, false);
        const uint32_t lead = seq_lead(sv), wfirst = lead >> 4;
        if (mine) { // stage the read's code words (prefetched ones first), wipe the bitmaps
            const uint32_t nw = n_words(sv);
            if (pf_valid) bad |= pf_bad; // (the words are in place: written behind the last turn's key phase)
            else {
                for (uint32_t t = tid; t < nw; t += UQ_THREADS) {
                    uint32_t b;
                    words[t] = load_code_word(sv, (uint64_t) wfirst + t, b);
                    bad |= b;
                }
            }
            uint4 *za = reinterpret_cast<uint4 *>(bmA), *zb = reinterpret_cast<uint4 *>(bmB);
#pragma unroll
            for (uint32_t z = 0; z < UQ_BM_WORDS / 4 / (uint32_t) UQ_THREADS; z++) { // (2^16 bits = 512 x 16 bytes)
                za[tid + z * UQ_THREADS] = make_uint4(0u, 0u, 0u, 0u);
                zb[tid + z * UQ_THREADS] = make_uint4(0u, 0u, 0u, 0u);
            }
        }
        lds_barrier();
        const bool has_nn = r_nn < a.n_queue;
        // the header of the read after next, and the list entry of the read behind it: requested now, looked at at the end of this turn
        const uint32_t r_n3 = uniform_u32(misc[6]);
        const uint32_t rs_n3 = r_n3 < a.n_queue ? seq_of(r_n3) : 0u;
        const uint64_t nn_o0 = has_nn ? a.offsets[rs_nn] : 0ull, nn_o1 = has_nn ? a.offsets[rs_nn + 1] : 0ull;
        // the next read's chunks: requested now, they land in LDS under the key phase and become code words behind it
        // (round 2 requested them behind the key phase and converted them on the spot: 12 % of a read's turn in that wait).
        // Requested by an instruction the compiler does not count (chunk16_to_lds_uncounted): behind the builtin it put `vmcnt(0)` in
        // front of every ds_* of the key phase, and each wave sat out the HBM round trip at the top of the phase that was to hide it.
        // The one wait for them is vm_wait_lds_loads() behind the key phase; a thread then reads the 16 bytes its own lane asked for.
        uint32_t nwn = 0, wfn = 0;
        if (nv_mine) {
            nwn = n_words(nv);
            wfn = seq_lead(nv) >> 4;
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const uint32_t tw = (uint32_t) tid + (uint32_t) u * UQ_THREADS;
                if (tw < nwn && chunk_is_plain(nv, (uint64_t) wfn + tw))
                    chunk16_to_lds_uncounted(nv.base + (nv.begin & ~15ull) + 16 * ((uint64_t) wfn + tw),
                                             lds_addr(smem) + RAW_OFF + (uint32_t) (wave + u * (UQ_THREADS / 64)) * 1024u);
            }
        }
        uint64_t rk[UQ_KREG];
        // the bitmap index of a key is a function of the key: computed again where the B bit is looked at instead of kept in
        // twenty registers (the kernel sits at its 128: 33 spilled vector registers with the indices kept)
        // (one multiplication of the folded key, by another constant than mix32's: the keys that share a bit of the bitmap must not
        //  share a bucket of the collision groups' sort; round 3's form ran the key through mix32 first: 8 instructions, twice per key)
        auto bm_index = [&](uint64_t key) -> uint32_t {
            return (((uint32_t) key ^ (uint32_t) (key >> 32)) * 0x85EBCA6Bu) >> (32 - UQ_BM_BITS);
        };
        // Register slots 4 g .. 4 g + 3 of all threads stand for places [4 UQ_THREADS g, 4 UQ_THREADS (g + 1)): a read of `span` places
        // (its k-mers behind the lead of its first word) fills the first ceil(span / (4 UQ_THREADS)) groups and no slot of the others,
        // for every thread alike -- a scalar compare per group and phase, and an empty group issues nothing (it used to run its LDS
        // reads, compares, ballots and branch skeletons for nothing: the mean read of the first shape fills 2.6 of its 5 groups).
        // Both phases skip by this one test: rk[] of a skipped group holds no key and is not looked at.
        const uint32_t span = uniform_u32(nk + (lead - 16u * wfirst));
        // A wave owns 256 consecutive places of a group, from 4 (UQ_THREADS g + 64 wave) on, and a read ends inside one wave: the waves
        // behind that one have no k-mer in this group and in all later ones.  The test is made for the wave's own first place -- it
        // contains the group's (wave 0's place is the group's first) and stays one scalar compare: the wave's number is read off the
        // first lane here, once per read (kept from the kernel's top it would be one more scalar register live around the read loop).
        const uint32_t wave_first = 256u * uniform_u32((uint32_t) tid >> 6);
        auto group_used = [&](int q0) -> bool { return 4u * (uint32_t) UQ_THREADS * (uint32_t) (q0 >> 2) + wave_first < span; };
        bool over = false; // uniform: too many keys in collision groups
        if (mine) {
            // ---- keys: extract, closure, bitmaps; the four ds_or_rtn of a slot group in flight together (in the compiled kernel: back to
            // back, one counted wait behind them; no vmcnt wait in the phase -- scripts/asm_mix.py --lds-waits) ----
            // (FAST: the closure of the headline -- canonical Kmer64bit through int64_hash, datasketcher.rs:225 -- without the
            //  per-key walk through apply_fhash's cases: the mode is the same for every key of the launch, and a chain of scalar
            //  compares and taken branches per key costs a workgroup of four waves per SIMD more than the arithmetic it selects)
            const uint32_t l0 = lead - 16u * wfirst; // place of the read's first base
            auto key_phase = [&](auto fast_tag) __attribute__((always_inline)) {
                constexpr bool FAST = decltype(fast_tag)::value;
                // (k-mer mask and shift are formed HERE, once per read: formed in front of the read loop they were spilled across it and
                //  reloaded -- three v_readlane_b32 and their s_nop -- for every key)
                const int kq = (int) opaque_u32((uint32_t) k);
#pragma unroll
                for (int q0 = 0; q0 < UQ_KREG; q0 += 4) {
                    if (!group_used(q0)) {
                        // (no instruction: the slots are told to hold nothing in particular.  Left alone they would carry the last
                        //  read's keys around the read loop -- forty registers live through staging, prefetch and collision sort:
                        //  101 / 66 spilled vector registers instead of 0 / 3)
#pragma unroll
                        for (int u = 0; u < 4; u++) rk[q0 + u] = __builtin_nondeterministic_value(rk[q0 + u]);
                        continue;
                    }
                    uint32_t bit[4], rbw[4], rbb[4]; // a slot's word of the bitmap and its bit there
                    const uint32_t wi = ((uint32_t) tid >> 2) + (uint32_t) (UQ_THREADS / 4) * (uint32_t) (q0 >> 2); // the quarter's word
                    const StepWin sw = step_win(words[wi], words[wi + 1], words[wi + 2], kq);
                    // (round 4, measured and not kept: a branch-free form for the waves whose quarters are whole -- 10.6 against 10.1 ms
                    //  per launch, 19 instead of 15 spilled registers)
#pragma unroll
                    for (int u = 0; u < 4; u++) {
                        const int q = q0 + u;
                        // a slot without a key ORs nothing into a word of its thread's own (one word for all such lanes of a wave
                        // would serialise them): the four ds_or_rtn below then stand outside every per-lane branch
                        rbw[u] = (uint32_t) tid;
                        rbb[u] = 0;
                        rk[q] = 0;
                        if (place_of(q) - l0 < nk) {
                            uint64_t val, rc;
                            step_val_rc_lane(sw, 4u * ((uint32_t) tid & 3u) + (uint32_t) u, val, rc);
                            const uint64_t key = FAST ? int64_hash(rc < val ? rc : val) : apply_fhash(cfg, val, rc);
                            rk[q] = key;
                            const uint32_t bi = bm_index(key);
                            rbw[u] = bi >> 5;
                            rbb[u] = 1u << (bi & 31u);
                        }
                    }
                    // the four round trips leave back to back; an answer is looked at when all four are out (inside the branch that
                    // issued it, the answer was waited for there: four dependent round trips per group)
#pragma unroll
                    for (int u = 0; u < 4; u++) bit[u] = atomicOr(&bmA[rbw[u]], rbb[u]);
#pragma unroll
                    for (int u = 0; u < 4; u++) bit[u] &= rbb[u];
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        if (bit[u]) atomicOr(&bmB[rbw[u]], bit[u]);
                }
            };
            if (cfg.fhash == KMU_FHASH_CANON_INVHASH && cfg.kmer_type == KMU_KMER64BIT) key_phase(std::true_type{});
            else key_phase(std::false_type{});
            lds_barrier();
        }
        // ---- the next read's chunks have landed: its code words replace this read's (every key of this read is in a register by
        // now -- the barrier behind the key phase -- and nothing below looks at `words`).  Round 5: they used to wait in three registers
        // per thread until the top of the next turn, in a kernel that sits on its register limit ----
        if (nv_mine) {
            vm_wait_lds_loads();
            pf_bad = 0;
#pragma unroll
            for (int u = 0; u < 3; u++) {
                const uint32_t tw = (uint32_t) tid + (uint32_t) u * UQ_THREADS;
                uint32_t b = 0;
                if (tw < nwn)
                    words[tw] = chunk_is_plain(nv, (uint64_t) wfn + tw)
                                    ? code_word_from_chunk(nv, (uint64_t) wfn + tw, *reinterpret_cast<const u32x4 *>(rawp + (size_t) tw * 16), b)
                                    : load_code_word(nv, (uint64_t) wfn + tw, b);
                pf_bad |= b;
            }
        }
        const uint64_t lb = sv.begin - off_first; // list entries of read r start here
        if (mine) {
            // ---- sort out: B bit clear = occurs once = list entry (key, 1) from the register; else collect ----
            // (r03: all twenty B bits read at once and ONE atomic pair per wave instead of five -- 15.9 against 13.0 ms per launch:
            //  the kernel sits at its 128 registers, twenty more live values spill)
#pragma unroll
            for (int q0 = 0; q0 < UQ_KREG; q0 += 4) {
                if (!group_used(q0)) continue; // (its rk[] hold no key: the key phase skipped it by the same test)
                bool uq[4], co[4];
                uint64_t um[4], cm[4];
                uint32_t ut = 0, ct = 0, bw[4];
                // the four B words are read by every lane (a slot without a key holds key 0: some word of the bitmap) and looked at
                // together: one wait per group
#pragma unroll
                for (int u = 0; u < 4; u++) bw[u] = bmB[bm_index(rk[q0 + u]) >> 5];
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const int q = q0 + u;
                    const bool have = place_of(q) - (lead - 16u * wfirst) < nk;
                    co[u] = have && (bw[u] & (1u << (bm_index(rk[q]) & 31u))) != 0u;
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
            const uint32_t n_u = uniform_u32(misc[0]), n_c = uniform_u32(misc[1]);
            over = n_c > UQ_COLL;
            if (!over && n_c) {
                // ---- the collision groups: counting sort on 10 hash bits, equal keys hand their weight to the first ----
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
                { // exclusive scan of the 1 024 bucket counts, two per thread
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
                uint32_t *lst_w = KMU_COLD_ARG(lst_w);
                for (uint32_t i = tid; i < n_c; i += UQ_THREADS) {
                    a.lst_keys[lb + n_u + i] = dk[i];
                    lst_w[lb + n_u + i] = dw[i];
                }
                bst[2 * tid] = 0;
                bst[2 * tid + 1] = 0;
            }
            if (tid == 0 && !over) { KMU_COLD_ARG(lst_n)[rs] = n_u + n_c; KMU_COLD_ARG(lst_nu)[rs] = n_u; }
        }
        if (tid == 0) {
            if (nk == 0) KMU_COLD_ARG(lst_n)[rs] = 0u; // no k-mer: k_pmh_points writes the row of an empty multiset
            else if (!mine || over) {       // the next kernel's: longer than the registers, or too repetitive
                KMU_COLD_ARG(lst_n)[rs] = 0u;
                KMU_COLD_ARG(redo_list)[atomicAdd(KMU_COLD_ARG(queue) + 56, 1u)] = rs;
            }
        }
        if (bad) atomicOr(KMU_COLD_ARG(err), DERR_NON_ACGT);
        pf_valid = nv_mine;
        r = r_next;
        rs = rs_next;
        sv = nv;
        r_next = r_nn;
        rs_next = rs_nn;
        r_nn = r_n3;
        rs_nn = uniform_u32(rs_n3);
        nv_mine = false;
        // (measured and not kept: the header words looked at on every path, which takes the compiler's `vmcnt(0)` -- pending on the path
        //  without a read after next -- from the top of the next turn: 7.58-7.59 against 7.57-7.59 ms per launch)
        if (has_nn) {
            nv.begin = uniform_u64(nn_o0);
            nv.len = uniform_u64(nn_o1) - nv.begin;
            nv_mine = fits(nv);
        }
        lds_barrier();
    }
}

// the forms the host side launches (kmu_sketch_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__(SketchArgs);
KMU_PMH_UQ_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

// kmu_pmh_general.hip -- the general per-sequence sketch kernel k_sketch_pmh3a (ProbMinHash3a / bottom-k, every input form) for gfx950.
//
// Reference loop being replaced (src/sketching/seqsketchjaccard.rs:224-243, setsketchert.rs:121-157):
//     for every read (rayon):  FnvHashMap<Val,u64> of fhash(kmer) over all k-mers  ->  ProbMinHash3a(m)
// MI355X mapping: one persistent workgroup per CU pulls reads from an atomic queue.  The read's weighted
// multiset is built in LDS by a counting sort on a 12-bit hash bucket: every k-mer takes a rank in its bucket with
// one ds_add_rtn, an in-place scan turns the bucket counts into starts, the keys are placed densely (dk[], dw[] = 1)
// and every key then looks for an earlier equal key inside its own (short) bucket segment -- a repeat zeroes its own
// weight and adds one to the first occurrence.  No compare-and-swap probing: the divergent probe loop of a hash
// table cost ~250 wave instructions per 64 k-mers on this VALU-bound kernel.  Reads with more k-mers than the dense
// arrays hold (~10.6 k) are processed in P hash-partitions (a key always lands in one partition, so counts stay
// exact).  The m slot minima (h as order-preserving f64 bits, arg-min key) stay in LDS across passes.
// Integer / f64 ALU + LDS only; HBM traffic = the read's bases in, m signatures out.
#include <algorithm>
#include <cmath>

#include "kmu_pmh_steps.h"

namespace kmu {

__device__ __forceinline__ uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t) (((uint64_t) a * b) >> 32); }

// The per-workgroup scratch lists live in global memory and are re-used read after read: a plain load can be served
// by a stale line of this CU's vector L1 (stores write through to L2 without refreshing it), so every read of them
// bypasses L1 (agent-scope load, `sc1`).
template <typename T>
__device__ __forceinline__ T ld_scr(const T *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// ... and every write is a write-through store (`sc1`), completed (vmcnt(0)) by the workgroup barrier that precedes
// the reads: the "sc1 stores and loads on both sides" hand-off form of the CDNA guide.
template <typename T>
__device__ __forceinline__ void st_scr(T *p, T v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// in-place exclusive scan of bst[0..NBUCKETS); bst[NBUCKETS] = total.  wtot: one word per wave.
// Four waves do it, sixteen counters per thread moved as 16-byte LDS words: the scan is pure bookkeeping that every
// pass pays, and with all sixteen waves on it the instruction count is four times higher for the same LDS traffic
// (the other waves simply wait at the barrier).  bst must be 16-byte aligned.
__device__ __forceinline__ void bucket_scan(uint32_t *bst, uint32_t *wtot) {
    static_assert(NBUCKETS == 4096, "256 threads x 16 counters");
    const int tid = threadIdx.x;
    uint4 c[4];
    uint32_t sum = 0, incl = 0;
    if (tid < 256) {
        const uint4 *src = reinterpret_cast<const uint4 *>(bst) + 4 * tid;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            c[q] = src[q];
            sum += c[q].x + c[q].y + c[q].z + c[q].w;
        }
        incl = wave_incl_scan_u32(sum);
        if (lane_id() == 63) wtot[tid >> 6] = incl;
    }
    __syncthreads();
    if (tid < 256) {
        uint32_t run = incl - sum;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const uint32_t v = wtot[w];
            run += w < (tid >> 6) ? v : 0u;
        }
        uint4 *dst = reinterpret_cast<uint4 *>(bst) + 4 * tid;
#pragma unroll
        for (int q = 0; q < 4; q++) {
            uint4 o;
            o.x = run; run += c[q].x;
            o.y = run; run += c[q].y;
            o.z = run; run += c[q].z;
            o.w = run; run += c[q].w;
            dst[q] = o;
        }
        if (tid == 255) bst[NBUCKETS] = run;
    }
    __syncthreads();
}

// the same economy for wiping the counters: four waves, 16-byte stores
__device__ __forceinline__ void bucket_clear(uint32_t *bst) {
    const int tid = threadIdx.x;
    if (tid < 256) {
        uint4 *dst = reinterpret_cast<uint4 *>(bst) + 4 * tid;
#pragma unroll
        for (int q = 0; q < 4; q++) dst[q] = make_uint4(0u, 0u, 0u, 0u);
        if (tid == 0) bst[NBUCKETS] = 0u;
    }
}

// One workgroup = one read at a time (all blocks of it in block mode).
// BOTTOMK = false: ProbMinHash3a on the multiset.  BOTTOMK = true: the multiset of hasher(fhash(kmer)) is sorted by
// the top bits of the hash itself, so the `m` smallest distinct hashes sit in the leading buckets; their exact rank
// (= output position) is "distinct keys in earlier buckets + smaller distinct keys in the own bucket".
//
// A partition pass normally sorts all its k-mer occurrences at once (SINGLE).  If the occurrences do not fit the dense
// arrays -- repetitive reads: poly-A, tandem repeats -- the pass is redone in ROUNDS of cap/2 positions; after every
// round the distinct (key, weight) pairs are compacted into a carry list that joins the next round's sort with its
// weights.  If even the distinct keys do not fit, the block is restarted with twice as many partitions.
// (A variant with the closure and k-mer type as template constants was tried: the hashing loop gets 18 % shorter, but
// the allocator then spills loop-carried state around the read header and the kernel as a whole is slower.)
// EMIT: stop after the multiset and write the distinct (key, weight) pairs of the read to global lists (k_pmh_points
// generates the points from there, one wave per read at full occupancy) instead of running pass B here.
// PLAIN: whole unpacked sequences to signature rows (the throughput case): the packed-input, block and partial-row paths
// are compiled out of that instantiation.  (Fixing the closure and the k-mer type as well was measured again on top of
// it: 93.7 against 89.1 ms -- the allocator trades the shorter hashing code for spills elsewhere.)
template <bool AA, bool BOTTOMK, bool EMIT, bool PLAIN>
__global__ void __launch_bounds__(1024) k_sketch_pmh3a(SketchArgs a) {
    static_assert(!(EMIT && PLAIN), "no route emits lists from the PLAIN form: those reads take k_multiset_uq");
    if constexpr (PLAIN) { // the compiler sees constants wherever these are read below
        a.packed = 0;
        a.block_size = 0;
        a.part_h = nullptr;
        a.part_k = nullptr;
        a.packed_offsets = nullptr;
    }
    const KmerCfg cfg = a.cfg;
    const bool sig32 = a.sig_bytes == 4;
    // the headline's closure (canonical Kmer64bit through int64_hash) without the walk through apply_fhash's cases per key (see k_multiset_uq)
    const bool fast64 = !AA && cfg.fhash == KMU_FHASH_CANON_INVHASH && cfg.kmer_type == KMU_KMER64BIT;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t cap = a.cap;
    uint64_t *dk = reinterpret_cast<uint64_t *>(smem); // dense keys of the current pass, grouped by bucket
    uint64_t *hmin = dk + cap;
    uint64_t *sig = hmin + a.m;
    uint32_t *dw = reinterpret_cast<uint32_t *>(sig + a.m); // weights (0 = repeat of an earlier entry)
    uint32_t *bst = dw + cap;                                // NBUCKETS + 1: counts, then starts
    uint32_t *misc = bst + NBUCKETS + 1;
    misc += (8 - ((NBUCKETS + 1) & 7)) & 7; // keep the u64 at misc[M_QMAX] 8-byte aligned
    uint32_t *wtot = misc + M_WORDS;
    uint32_t *defc = wtot + 16; // keys set aside for partition p + 1 (DEF_PARTS counters)
    uint32_t *words = defc + DEF_PARTS;
    words += (4 - ((uintptr_t) words >> 2 & 3)) & 3; // 16-byte aligned: raw chunks are parked here as uint4
    uint64_t *qmax_sh = reinterpret_cast<uint64_t *>(&misc[M_QMAX]);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid >> 6, nwaves = nthreads >> 6;
    const int k = cfg.k;
    const uint32_t tile_pos = (a.tile_words - 2) * 16; // k-mer start positions covered by one staged tile
    uint64_t *scr_keys = a.scr_keys + (uint64_t) blockIdx.x * cap;
    uint32_t *scr_info = a.scr_info + (uint64_t) blockIdx.x * cap;
    uint32_t *scr_w = a.scr_w + (uint64_t) blockIdx.x * cap;
    uint64_t *def_keys = a.def_keys + (uint64_t) blockIdx.x * DEF_CAP;
    // bottom-k: the running list of the m smallest hashes re-uses the LDS of the (unused) slot minima
    uint64_t *bk_keys = hmin;
    uint32_t *bk_cnt = reinterpret_cast<uint32_t *>(sig);
    uint32_t bk_n = 0; // entries of the bottom-k running list (uniform)
    uint32_t emit_n = 0; // EMIT: list entries of the current read written by earlier passes (uniform)

    bucket_clear(bst);
    for (int s = tid; s < a.m; s += nthreads) { hmin[s] = H_INIT; sig[s] = 0; }
    if (tid == 0) { misc[M_NSCR] = 0; misc[M_DEF] = 0; misc[M_FLAGS] = 0; misc[M_FLAGS + 1] = 0; *qmax_sh = H_INIT; }
    // reads are taken from the global queue QCHUNK at a time (thread 0 keeps the cursor): one same-address atomic per
    // read would cap the whole grid at the L2's rate for a single address
    // The next chunk is requested while the last read of the current one is still to be handed out, so its latency is
    // never waited for.
    // (k_sketch_smallk keeps the same cursor, and both kernels spell it out: as a shared function its ask-ahead test is simplified on its
    //  own before it is inlined, which changes the scalar code around it in one kernel or the other -- by reference k_sketch_pmh3a's,
    //  by value k_sketch_smallk's)
    uint32_t q_next = 0, q_end = 0, q_pend = 0;
    bool q_pending = false;
    if (tid == 0) {
        q_next = atomicAdd(a.queue, (uint32_t) QCHUNK);
        q_end = q_next + QCHUNK;
        misc[M_READ] = q_next++;
    }
    __syncthreads();
    auto seq_of = [&](uint32_t q) -> uint32_t { return (!PLAIN && a.read_list) ? uniform_u32(a.read_list[q]) : q; };
    auto view_of = [&](uint32_t q) { return seq_view_of(a, seq_of(q)); };
    // number of staged code words of a read's very first tile (block 0, positions from 0)
    auto first_tile_words = [&](const SeqView &v) -> uint32_t {
        const uint64_t nka = v.len >= (uint64_t) k ? v.len - k + 1 : 0;
        uint64_t pe0 = a.block_size ? (uint64_t) a.block_size : nka;
        if (pe0 > nka) pe0 = nka;
        if (pe0 == 0) return 0u;
        const uint64_t t1 = pe0 < (uint64_t) tile_pos ? pe0 : (uint64_t) tile_pos;
        const uint32_t ld = seq_lead(v);
        return (uint32_t) (((t1 - 1 + ld + (uint64_t) k - 1) >> 4) - (uint64_t) (ld >> 4) + 1) + 2;
    };
    // The NEXT read's header is fetched as soon as its index is known, and the first 16 chunks x 64 lanes x 16 waves of its
    // bases are requested while this read's duplicates are merged (A3): HBM -> LDS directly, raw, into the `words` area
    // (free from there on).  A fresh read starts without waiting for HBM.  pf_r = the read whose head sits there.
    SeqView nv;
    nv.base = a.bases; nv.begin = 0; nv.len = 0; nv.total = 0; nv.packed = a.packed;
    uint32_t flag_sel = 0; // uniform
    uint32_t nv_r = 0xFFFFFFFFu, pf_r = 0xFFFFFFFFu, pf_nw = 0;
    u32x4 raw_pf = (u32x4) (0u); // PLAIN: this thread's parked chunk of the next read
    lds_barrier();
    uint32_t r = uniform_u32(misc[M_READ]);
    while (r < a.n_queue) {
        // Thread 0 takes the next read now (the atomic's latency hides under this read's work), posts it in
        // misc[M_NEXT] before the first barrier after the ranks are taken, and everybody picks it up behind that barrier.
        uint32_t r_next = 0, r_follow = 0xFFFFFFFFu;
        bool next_posted = false;
        if (tid == 0) {
            if (q_next == q_end) {
                if (!q_pending) q_pend = atomicAdd(a.queue, (uint32_t) QCHUNK);
                q_next = q_pend;
                q_end = q_pend + QCHUNK;
                q_pending = false;
            }
            r_next = q_next++;
            if (q_next == q_end && !q_pending) { // used one read from now
                q_pend = atomicAdd(a.queue, (uint32_t) QCHUNK);
                q_pending = true;
            }
        }
        const SeqView sv = nv_r == r ? nv : view_of(r);
        // positions inside a read are 32-bit from here on (half the scalar registers, half the vector instructions per
        // index computation); a single sequence of 2^31 bases or more is refused
        if (sv.len >= 0x80000000ull && tid == 0) atomicOr(a.err, DERR_TABLE_FULL);
        const uint32_t L = sv.len >= 0x80000000ull ? 0u : (uint32_t) sv.len;
        const uint32_t nk_all = L >= (uint32_t) k ? L - (uint32_t) k + 1u : 0u;
        if (L == 0 && tid == 0 && !a.hashed_bytes) atomicOr(a.err, 8u); // an empty list of pre-hashed values is fine
        if (nk_all == 0 && !a.hashed_bytes && wave_validate_seq(sv, wave, nwaves, AA))
            atomicOr(a.err, AA ? DERR_BAD_AA : DERR_NON_ACGT);
        const uint32_t lead = AA ? 0u : seq_lead(sv);
        // blocks of the read (src/sketching/seqblocksketch.rs:108-146); whole read = one block
        const uint32_t B = a.block_size ? a.block_size : (nk_all ? nk_all : 1u);
        uint32_t nblocks = a.block_size ? (uint32_t) (((uint64_t) L + B - 1) / B) : 1u;
        if (a.skip_longer && nk_all > a.skip_longer) nblocks = 0; // its row comes from the global path
        for (uint32_t blk = 0; blk < nblocks; blk++) {
            const uint64_t pb64 = (uint64_t) blk * B, pe64 = pb64 + B;
            const uint32_t pb = pb64 > nk_all ? nk_all : (uint32_t) pb64, pe = pe64 > nk_all ? nk_all : (uint32_t) pe64;
            const uint32_t nk = pe - pb;
            // number of hash partitions: any P with nk / P comfortably below the dense capacity will do (the multiset is
            // exact for every P), so no 64-bit division: a product with the reciprocal, rounded up
            uint32_t P = nk == 0 ? 0u : nk <= a.part_target ? 1u : (uint32_t) ((double) nk * a.inv_part_target) + 1u;
            uint32_t bad = 0;
            bool full = false;
            bool redo = false; // uniform; PLAIN only
            // k-mer occurrences of positions [q0, q1) that belong to partition `part` take a bucket rank; the first
            // KREG * nthreads positions of a SINGLE pass keep their key in registers, the rest goes to the scratch.
            // A block that needs several partition passes is scanned (extracted, hashed) ONCE: pass 0 sets the keys of the
            // later partitions aside in a global list, the later passes read their keys from there.
            bool def_valid = false; // uniform
            for (bool block_done = (P == 0); !block_done;) {
                bool restart_block = false; // uniform
                def_valid = false;
                for (uint32_t part = 0; part < P && !restart_block; part++) {
                    bool rounds_mode = false; // uniform
                    for (bool part_done = false; !part_done;) {
                        uint64_t rk[KREG];
                        uint32_t rb[KREG];
#pragma unroll
                        for (int q = 0; q < KREG; q++) rb[q] = 0xFFFFFFFFu; // (rk[q] is read only where rb[q] names a key)

                        const uint32_t round_len = rounds_mode ? cap / 2 : nk;
                        uint32_t carry_n = 0; // distinct (key, weight) pairs carried from earlier rounds (in scr_*)
                        if (BOTTOMK && part > 0) { // the running list of the earlier partitions travels as carry
                            for (uint32_t i = tid; i < bk_n; i += nthreads) { st_scr(&scr_keys[i], bk_keys[i]); st_scr(&scr_w[i], bk_cnt[i]); }
                            carry_n = bk_n;
                            __syncthreads();
                        }
                        bool overflow = false; // uniform
                        for (uint32_t q0 = pb; q0 < pe && !overflow; q0 += round_len) {
                            const uint32_t q1 = pe - q0 > round_len ? q0 + round_len : pe;
                            const bool last_round = q1 == pe;
                            if (!PLAIN && carry_n) { // carried pairs take their ranks first (misc[M_NSCR] is 0 between passes)
                                if (tid == 0) misc[M_NSCR] = carry_n;
                                for (uint32_t i = tid; i < carry_n; i += nthreads) {
                                    const uint64_t key = ld_scr(&scr_keys[i]);
                                    const uint32_t b = BOTTOMK ? (uint32_t) (key >> a.bk_shift) & (NBUCKETS - 1)
                                                               : mix32(key) >> (32 - BUCKET_BITS);
                                    st_scr(&scr_info[i], (b << 16) | atomicAdd(&bst[b], 1u));
                                }
                                __syncthreads(); // orders the scratch stores above
                            }
                            // ---- A1: bucket ranks of the keys of this partition in [q0, q1) ------------------------
                            // this pass fills the sub-lists (one per later partition; more partitions than sub-lists: rescan)
                            const bool defer_on = !BOTTOMK && P > 1 && P <= DEF_PARTS + 1 && part == 0 && !rounds_mode;
                            const bool from_list = !BOTTOMK && part > 0 && !rounds_mode && def_valid;
                            if (defer_on) {
                                if ((uint32_t) tid < DEF_PARTS) defc[tid] = 0;
                                if (tid == 0) misc[M_DEF] = 0; // becomes 1 if a sub-list overflows
                                lds_barrier();
                            }
                            if (from_list) {
                                const uint32_t seg_n = uniform_u32(defc[part - 1]);
                                const uint64_t *seg = def_keys + (uint64_t) (part - 1) * DEF_SEG;
                                for (uint32_t i = tid; i < seg_n; i += nthreads) {
                                    const uint64_t key = ld_scr(&seg[i]);
                                    const uint32_t b = mix32(key) >> (32 - BUCKET_BITS);
                                    const uint32_t rank = atomicAdd(&bst[b], 1u);
                                    if (rank < 65536u) { // (a pass of a partitioned block parks its keys: use_park)
                                        const uint32_t si = atomicAdd(&misc[M_NSCR], 1u);
                                        if (si < (uint32_t) KREG * nthreads && si < cap) { dk[si] = key; dw[si] = (b << 16) | rank; }
                                    }
                                }
                            }
                            const uint32_t ntiles = from_list ? 0u : AA ? 1u : (uint32_t) (((uint64_t) (q1 - q0) + tile_pos - 1) >> a.tile_shift); // tile_pos is a power of two
                            for (uint32_t tile = 0; tile < ntiles; tile++) {
                                const uint32_t tp0 = AA ? q0 : q0 + tile * tile_pos;
                                const uint32_t tp1 = AA ? q1 : (q1 - tp0 > tile_pos ? tp0 + tile_pos : q1);
                                uint32_t wfirst = 0;
                                if (!AA) {
                                    wfirst = (tp0 + lead) >> 4;
                                    const uint32_t wlast = (uint32_t) (((uint64_t) tp1 - 1 + lead + (uint64_t) k - 1) >> 4);
                                    const uint32_t nw = (wlast - wfirst + 1) + 2;
                                    // the raw chunks of words [0, pf_nw) may have been parked here by the previous read
                                    const bool parked = pf_r == r && tp0 == 0 && (uint32_t) tid < pf_nw;
                                    pf_r = 0xFFFFFFFFu;
                                    u32x4 raw = (u32x4) (0u);
                                    if (PLAIN) {
                                        // the parked chunk was taken to registers behind the last barrier of the previous
                                        // read; a pass's first tile follows a barrier that every reader of `words` has
                                        // passed, so only the later tiles wait here
                                        if (parked) raw = raw_pf;
                                        if (tile != 0) lds_barrier();
                                    } else {
                                        if (parked) raw = reinterpret_cast<const u32x4 *>(words)[tid];
                                        lds_barrier(); // the previous user of `words` is done
                                    }
                                    for (uint32_t t = tid; t < nw; t += nthreads) {
                                        uint32_t b;
                                        words[t] = (parked && t == (uint32_t) tid && chunk_is_plain(sv, wfirst + t))
                                                       ? code_word_from_chunk(sv, wfirst + t, raw, b)
                                                       : load_code_word(sv, wfirst + t, b);
                                        bad |= b;
                                    }
                                    lds_barrier();
                                }
                                for (uint32_t pr = tp0; pr < tp1; pr += (uint32_t) KREG * nthreads) {
                                    // Where a key waits for the scan: in registers (one pass over a read that fits: its first
                                    // KREG * nthreads positions), parked unsorted in the still unused dense arrays (a pass of
                                    // a partitioned read keeps 1/P of the positions it scans), else in the global scratch.
                                    const bool use_park = !rounds_mode && P > 1 && (PLAIN || carry_n == 0);
                                    const bool use_regs = !rounds_mode && !use_park && tile == 0 && pr == tp0;
#pragma unroll
                                    for (int q = 0; q < KREG; q++) {
                                        const uint32_t p = pr + (uint32_t) q * nthreads + tid;
                                        if (p < tp1) {
                                            uint64_t val, rc = 0;
                                            if (AA && a.hashed_bytes) {
                                                val = a.hashed_bytes == 4
                                                          ? (uint64_t) reinterpret_cast<const uint32_t *>(a.hashed)[sv.begin + p]
                                                          : reinterpret_cast<const uint64_t *>(a.hashed)[sv.begin + p];
                                            } else if (AA) {
                                                val = 0;
                                                for (int j = 0; j < k; j++) {
                                                    uint32_t c = code_aa(sv.base[sv.begin + p + j]);
                                                    bad |= c == 0;
                                                    val = (val << 5) | c;
                                                }
                                            } else {
                                                val = staged_kmer(words, p + lead - 16u * wfirst, k);
                                                rc = revcomp_val(val, k);
                                            }
                                            bool go = true;
                                            uint64_t key = 0;
                                            uint32_t h = 0;
                                            if (go) {
                                                key = (AA && a.hashed_bytes) ? val : fast64 ? int64_hash(rc < val ? rc : val) : apply_fhash(cfg, val, rc);
                                                if (BOTTOMK) key = hasher_finish(a.hasher, key, sig32);
                                                h = mix32(key);
                                                const uint32_t kp = P > 1 ? mulhi32(h * 0x85EBCA6Bu, P) : 0u;
                                                if (kp != part) {
                                                    go = false;
                                                    if (defer_on) { // its own pass will pick it up without re-hashing
                                                        const uint32_t di = atomicAdd(&defc[kp - 1], 1u);
                                                        if (di < DEF_SEG) st_scr(&def_keys[(uint64_t) (kp - 1) * DEF_SEG + di], key);
                                                        else misc[M_DEF] = 1u;
                                                    }
                                                }
                                            } else if (val == 0x1234567ull) full = true;
                                            if (go) {
                                                const uint32_t b = BOTTOMK ? (uint32_t) (key >> a.bk_shift) & (NBUCKETS - 1)
                                                                           : h >> (32 - BUCKET_BITS);
                                                const uint32_t rank = atomicAdd(&bst[b], 1u);
                                                if (rank < 65536u) { // else: the pass overflows and is redone in rounds
                                                    if (use_regs) { rk[q] = key; rb[q] = (b << 16) | rank; }
                                                    else {
                                                        const uint32_t si = atomicAdd(&misc[M_NSCR], 1u);
                                                        if (use_park) {
                                                            if (si < (uint32_t) KREG * nthreads && si < cap) { dk[si] = key; dw[si] = (b << 16) | rank; }
                                                        } else if (!PLAIN && si < cap) { st_scr(&scr_keys[si], key); st_scr(&scr_info[si], (b << 16) | rank); st_scr(&scr_w[si], 1u); }
                                                    }
                                                }
                                            } else if (h == 0x12345u) full = true;
                                        }
                                    }
                                }
                            }
                            if (tid == 0 && !next_posted) { misc[M_NEXT] = r_next; next_posted = true; }
                            __syncthreads();
                            if (defer_on) def_valid = uniform_u32(misc[M_DEF]) == 0u; // complete (every position scanned) if all fitted
                            // ---- A2: counts -> starts, dense placement ---------------------------------------------
                            r_follow = uniform_u32(misc[M_NEXT]);
                            if (nv_r != r_follow && r_follow < a.n_queue) { nv = view_of(r_follow); nv_r = r_follow; }
                            // parked keys move to the registers (the barriers of the scan separate this from the placement)
                            const bool parked_pass = !rounds_mode && P > 1 && (PLAIN || carry_n == 0);
                            const uint32_t n_park = parked_pass ? uniform_u32(misc[M_NSCR]) : 0u;
                            if (parked_pass && n_park <= (uint32_t) KREG * nthreads && n_park <= cap) {
#pragma unroll
                                for (int q = 0; q < KREG; q++) {
                                    const uint32_t idx = (uint32_t) q * nthreads + tid;
                                    if (idx < n_park) { rk[q] = dk[idx]; rb[q] = dw[idx]; }
                                }

                            }
                            bucket_scan(bst, wtot);
                            const uint32_t n_keys = uniform_u32(bst[NBUCKETS]);
                            // (PLAIN: a single pass keeps every key in registers -- the host checks part_target -- and a
                            //  partitioned one parks them: the scratch lists are not used)
                            const uint32_t n_scr = (PLAIN || parked_pass) ? 0u : uniform_u32(misc[M_NSCR]);
                            if (n_keys > cap || n_scr > cap || n_park > (uint32_t) KREG * nthreads || n_park > cap) overflow = true;
                            if (!overflow) {
                                // (all bucket starts are requested before the first store: a load behind a store to LDS
                                // cannot be moved up by the compiler, and ten dependent round trips are the phase)
#pragma unroll
                                for (int q = 0; q < KREG; q++)
                                    if (rb[q] != 0xFFFFFFFFu) {
                                        const uint32_t b = rb[q] >> 16;
                                        rb[q] = (b << 16) | (bst[b] + (rb[q] & 0xFFFFu));
                                    }
#pragma unroll
                                for (int q = 0; q < KREG; q++)
                                    if (rb[q] != 0xFFFFFFFFu) {
                                        const uint32_t pos = rb[q] & 0xFFFFu;
                                        dk[pos] = rk[q];
                                        dw[pos] = 1u;
                                    }
                                for (uint32_t i = tid; i < n_scr; i += nthreads) { // written by this workgroup: L2 hits
                                    const uint32_t info = ld_scr(&scr_info[i]);
                                    const uint32_t b = info >> 16, pos = bst[b] + (info & 0xFFFFu);
                                    dk[pos] = ld_scr(&scr_keys[i]);
                                    dw[pos] = ld_scr(&scr_w[i]);
                                }
                            }
                            __syncthreads();
                            // ---- A3: a key with an earlier equal key in its bucket segment hands its weight over ------
                            const bool do_pf = !AA && !BOTTOMK && !a.packed && !overflow && last_round && blk + 1 == nblocks &&
                                               part + 1 == P && nv_r == r_follow && r_follow < a.n_queue &&
                                               (size_t) a.tile_words * 4 >= (size_t) nthreads * 16;
                            if (do_pf) {
                                uint32_t n = first_tile_words(nv);
                                if (n > (uint32_t) nthreads) n = (uint32_t) nthreads; // the head only
                                const uint64_t wf = seq_lead(nv) >> 4;
                                if ((uint32_t) tid < n && chunk_is_plain(nv, wf + tid))
                                    chunk16_to_lds(nv.base + (nv.begin & ~15ull) + 16 * (wf + tid),
                                                   reinterpret_cast<uint8_t *>(words) + (size_t) wave * 1024);
                                pf_r = r_follow;
                                pf_nw = n;
                            }
                            if (!overflow) {
                                // rb[q] becomes (own position << 16) | cursor; the walks of a thread's keys advance together,
                                // five LDS reads in flight at a time, instead of one key after the other
#pragma unroll
                                for (int q = 0; q < KREG; q++) {
                                    uint32_t v = 0u; // invalid: cursor == position == 0
                                    if (rb[q] != 0xFFFFFFFFu) v = ((rb[q] & 0xFFFFu) << 16) | bst[rb[q] >> 16];
                                    rb[q] = v;
                                }
                                static_assert(KREG % 5 == 0, "the duplicate walk advances five keys at a time");
#pragma unroll
                                for (int q0 = 0; q0 < KREG; q0 += 5) {
                                    for (;;) {
                                        bool act[5];
                                        uint64_t kq[5];
                                        bool any_act = false;
#pragma unroll
                                        for (int u = 0; u < 5; u++) {
                                            act[u] = (rb[q0 + u] & 0xFFFFu) < (rb[q0 + u] >> 16);
                                            kq[u] = act[u] ? dk[rb[q0 + u] & 0xFFFFu] : 0ull;
                                            any_act |= act[u];
                                        }
                                        if (!__any(any_act)) break;
#pragma unroll
                                        for (int u = 0; u < 5; u++)
                                            if (act[u]) {
                                                if (kq[u] == rk[q0 + u]) {
                                                    dw[rb[q0 + u] >> 16] = 0u;
                                                    atomicAdd(&dw[rb[q0 + u] & 0xFFFFu], 1u);
                                                    rb[q0 + u] = 0u; // done
                                                } else rb[q0 + u]++;
                                            }
                                    }
                                }
#pragma unroll
                                for (int q = 0; q < KREG; q++) rb[q] = 0xFFFFFFFFu; // consumed (a later round must not see them)
                                for (uint32_t i = tid; i < n_scr; i += nthreads) {
                                    const uint32_t info = ld_scr(&scr_info[i]);
                                    const uint32_t b = info >> 16, pos = bst[b] + (info & 0xFFFFu);
                                    const uint64_t key = dk[pos];
                                    for (uint32_t j = bst[b]; j < pos; j++)
                                        if (dk[j] == key) {
                                            // the weight is only written here (by its owner) and read at the end
                                            const uint32_t wpos = __hip_atomic_exchange(&dw[pos], 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                                            atomicAdd(&dw[j], wpos);
                                            break;
                                        }
                                }
                            }
                            __syncthreads();
                            if (!PLAIN && !overflow && !last_round) {
                                // ---- compact the distinct pairs into the carry list (scr_keys / scr_w) ------------------
                                if (tid == 0) misc[M_NSCR] = 0;
                                __syncthreads();
                                for (uint32_t base = 0; base < n_keys; base += nthreads) { // uniform trip count (ballot)
                                    const uint32_t i = base + tid;
                                    const uint32_t w = i < n_keys ? dw[i] : 0u;
                                    const uint64_t cm = __ballot(w != 0u);
                                    if (cm) {
                                        const int leader = __ffsll((unsigned long long) cm) - 1;
                                        uint32_t basepos = 0;
                                        if (lane_id() == leader) basepos = atomicAdd(&misc[M_NSCR], (uint32_t) __popcll(cm));
                                        basepos = bcast_u32(basepos, leader);
                                        if (w != 0u) {
                                            const uint32_t pos = basepos + (uint32_t) __popcll(cm & ((1ull << lane_id()) - 1ull));
                                            st_scr(&scr_keys[pos], dk[i]);
                                            st_scr(&scr_w[pos], w);
                                        }
                                    }
                                }
                                __syncthreads();
                                carry_n = uniform_u32(misc[M_NSCR]);
                                if (carry_n > cap - cap / 2) overflow = true; // no room for another round of new k-mers
                                bucket_clear(bst);
                                __syncthreads();
                            }
                            if (!overflow && last_round) {
                                if (EMIT) {
                                    // ---- the pairs of this pass leave for the points kernel -------------------------------
                                    // a straight copy of the dense arrays, duplicates included with weight 0 (k_pmh_points
                                    // skips them): no compaction, no atomics.  emit_n = entries of this read so far (all
                                    // passes; at most one per k-mer, so the list of a read fits its bases' index range)
                                    const uint32_t rsq = seq_of(r); // (the general instantiation may be walking a list of reads)
                                    const uint64_t lbase = a.offsets[rsq] - a.offsets[0] + emit_n; // (a range of a larger read set)
                                    for (uint32_t i = tid; i < n_keys; i += nthreads) {
                                        a.lst_keys[lbase + i] = dk[i];
                                        a.lst_w[lbase + i] = dw[i];
                                    }
                                    emit_n += n_keys;
                                } else if (!BOTTOMK) {
                                    // ---- B1: the first point of every distinct key -------------------------------------
                                    uint32_t chunk = 0;
                                    bool any_deferred = false;
                                    for (uint32_t base = 0; base < n_keys; base += nthreads, chunk++) {
                                        const uint32_t i = base + tid;
                                        uint64_t key = 0;
                                        uint32_t w = 0;
                                        if (i < n_keys) { key = dk[i]; w = dw[i]; }
                                        const bool have = w != 0u;
                                        if (__any(have)) {
                                            const bool deferred = pmh3a_first_point(a, sig32, hmin, sig, qmax_sh, ((chunk + wave) & B1_REFRESH_MASK) == 0u, have, key, w);
                                            if (deferred) { dw[i] = w | 0x80000000u; any_deferred = true; }
                                        }
                                    }
                                    // ---- B2: more points for the remembered keys that still lie below q_max -----------
                                    // (a flag word in LDS, not __syncthreads_or: its library reduction brings static LDS,
                                    // which would cost the kernel its 160 KiB dynamic allocation; the word
                                    // alternates with every pass: it is cleared one pass after it was read)
                                    if (__any(any_deferred) && lane_id() == 0) misc[M_FLAGS + flag_sel] = 1u;
                                    lds_barrier();
                                    const bool run_b2 = uniform_u32(misc[M_FLAGS + flag_sel]) != 0u;
                                    flag_sel ^= 1u;
                                    if (tid == 0) misc[M_FLAGS + flag_sel] = 0u;
                                    if (run_b2) {
                                        uint64_t qb = wave_qmax(hmin, a.m);
                                        for (uint32_t base = 0; base < n_keys; base += nthreads) {
                                            const uint32_t i = base + tid;
                                            const uint32_t w = i < n_keys ? dw[i] : 0u;
                                            double winv = 0.0;
                                            bool alive = false;
                                            if (w & 0x80000000u) { // round 2 starts at h = winv * 1
                                                winv = 1.0 / (double) (w & 0x7FFFFFFFu);
                                                alive = winv < __longlong_as_double((long long) qb);
                                            }
                                            if (__any(alive)) pmh3a_more_points(a, sig32, hmin, sig, qb, alive, alive ? dk[i] : 0ull, winv);
                                        }
                                    }
                                } else {
                                    // ---- bottom-k selection: rank = distinct keys in earlier buckets + smaller ones in
                                    //      the own bucket ----------------------------------------------------------------
                                    uint32_t *dcnt = words; // the staged code words are no longer needed in this pass
                                    for (uint32_t b = tid; b < NBUCKETS; b += nthreads) {
                                        uint32_t d = 0;
                                        for (uint32_t j = bst[b]; j < bst[b + 1]; j++) d += dw[j] != 0u;
                                        dcnt[b] = d;
                                    }
                                    __syncthreads();
                                    bucket_scan(dcnt, wtot);
                                    const uint32_t n_distinct = uniform_u32(dcnt[NBUCKETS]);
                                    for (uint32_t i = tid; i < n_keys; i += nthreads) {
                                        if (dw[i] == 0u) continue;
                                        const uint64_t key = dk[i];
                                        const uint32_t b = (uint32_t) (key >> a.bk_shift) & (NBUCKETS - 1);
                                        uint32_t rnk = dcnt[b];
                                        if (rnk >= (uint32_t) a.m) continue;
                                        for (uint32_t j = bst[b]; j < bst[b + 1]; j++) rnk += (dw[j] != 0u) && dk[j] < key;
                                        if (rnk < (uint32_t) a.m) { bk_keys[rnk] = key; bk_cnt[rnk] = dw[i]; }
                                    }
                                    bk_n = n_distinct < (uint32_t) a.m ? n_distinct : (uint32_t) a.m;
                                    __syncthreads(); // bst / dk / dw are still being read until every thread is done
                                }
                            }
                            if (overflow || last_round) {
                                bucket_clear(bst);
                                if (tid == 0) misc[M_NSCR] = 0;
                                if (PLAIN && pf_r != 0xFFFFFFFFu) { // requested before A3: long landed
                                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                                    if ((uint32_t) tid < pf_nw) raw_pf = reinterpret_cast<const u32x4 *>(words)[tid];
                                }
                                lds_barrier(); // the points are final (-> signature row); bst is clean for the next pass
                            }
                        }
                        if (!overflow) part_done = true;
                        else if (PLAIN) { redo = true; restart_block = true; part_done = true; } // the general kernel's
                        else if (!rounds_mode) rounds_mode = true; // redo this partition round by round
                        else { restart_block = true; part_done = true; }
                    }
                }
                if (!restart_block) block_done = true;
                else if (PLAIN && redo) block_done = true;
                else if (P >= 65536u) { full = true; block_done = true; }
                else if constexpr (!PLAIN) {
                    // too many distinct keys per partition: start the block over with twice as many partitions
                    P *= 2;
                    for (int t = tid; t < a.m; t += nthreads) { hmin[t] = H_INIT; sig[t] = 0; }
                    if (tid == 0) *qmax_sh = H_INIT;
                    emit_n = 0; // (EMIT) the list of this read starts over
                    bk_n = 0;
                    __syncthreads();
                }
            }
            if (bad) atomicOr(a.err, AA ? DERR_BAD_AA : DERR_NON_ACGT);
            if (full) atomicOr(a.err, DERR_TABLE_FULL);
            if (BOTTOMK) {
                // rows: the m smallest distinct hashes ascending, padded with u64::MAX; counts wrap like the
                // reference's u16 / u8 (minhash.rs:87-96, :243-262)
                __syncthreads();
                for (int t = tid; t < a.m; t += nthreads) {
                    const bool have = (uint32_t) t < bk_n;
                    reinterpret_cast<uint64_t *>(a.sig_out)[(uint64_t) r * a.m + t] = have ? bk_keys[t] : 0xFFFFFFFFFFFFFFFFull;
                    if (a.counts_out) a.counts_out[(uint64_t) r * a.m + t] = have ? (bk_cnt[t] & a.bk_mask) : 0u;
                }
                bk_n = 0;
            } else if (EMIT) {
                if (tid == 0) a.lst_n[seq_of(r)] = emit_n; // the row is written by k_pmh_points
                emit_n = 0;
            } else {
                // ---- signature of this block: arg-min key per slot, initobj (0) for an empty multiset -----------
                const uint32_t rs = seq_of(r);
                uint64_t row = a.block_rows ? a.block_rows[rs] + blk : (uint64_t) rs;
                if (PLAIN && redo) { // nothing of this sequence is kept: the general kernel sketches it from scratch
                    __syncthreads(); // (points of earlier partitions may still be in flight)
                    for (int t = tid; t < a.m; t += nthreads) { hmin[t] = H_INIT; sig[t] = 0; }
                    if (tid == 0) {
                        *qmax_sh = H_INIT;
                        a.redo_list[atomicAdd(a.queue + 56, 1u)] = r;
                    }
                } else
                for (int t = tid; t < a.m; t += nthreads) {
                    if (a.part_h) {
                        a.part_h[row * a.m + t] = hmin[t];
                        a.part_k[row * a.m + t] = sig[t];
                    } else {
                        uint64_t v = hmin[t] == H_INIT ? 0ull : sig[t];
                        if (sig32) reinterpret_cast<uint32_t *>(a.sig_out)[row * a.m + t] = (uint32_t) v;
                        else reinterpret_cast<uint64_t *>(a.sig_out)[row * a.m + t] = v;
                    }
                    hmin[t] = H_INIT;
                    sig[t] = 0;
                }
                if (tid == 0) *qmax_sh = H_INIT;
                if (PLAIN && redo) __syncthreads();
            }
            // (no barrier: the row and the slots are touched again only behind the barriers of the next pass)
        }
        if (r_follow == 0xFFFFFFFFu) { // a read without a single pass (no k-mer)
            if (tid == 0) misc[M_NEXT] = r_next;
            lds_barrier();
            r_follow = uniform_u32(misc[M_NEXT]);
            lds_barrier();
        }
        r = r_follow;
    }
}

// the forms the host side launches (kmu_sketch_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__(SketchArgs);
KMU_PMH_GENERAL_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

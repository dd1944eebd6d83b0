// kmu_seed_chains.hip -- from minimizer hits (pairs of minimizer entries that carry the same hash) to one colinear chain per read
// pair, at base resolution and on the device (kmu_seed_chains; the contract is in include/kmu.h).  A pair (ea, eb) is an ANCHOR of
// the read pair (read_q[ea], read_db[eb]) with relative strand s, x = pos_q[ea] and y = +-pos_db[eb]; the anchors of one
// (read_a, read_b, s) are a GROUP, ordered by (x, y).
//
//  k_chain_keys   COUNT and WRITE: runs_compact of kmu_runs.h over ChainPairs, which says what a pair is.  decode: the gather of
//                 the six values, the range checks (a pair that fails one is never used as an index; it raises bad and the call
//                 is refused at its one synchronisation), the KMU_CHAIN_UPPER test.  store: anchor c keeps prim = read_a << 32 |
//                 read_b and sec = s << 63 | x << 32 | (y + ybias); sec is the first sort key, c the value.  ybias is 2^31, or
//                 max_pos where the caller promises one: the keys then differ in fewer bytes.
//  grouping       runs_order of kmu_runs.h with the strand bit of sec as the inner key: the order is (read_a, read_b, s, x, y),
//                 a GROUP is an inner unit.  Profiled as k_chain_gather, k_chain_heads, k_chain_starts.
//  k_chain_dp     one wave per group, groups dealt grid-stride.  The wave takes the anchors 64 at a time: lane l holds anchor
//                 c * 64 + l of chunk c in registers (x, y, f, start, n), and the same five of chunk c - 1.  The lookback window of
//                 anchor i = c * 64 + t is exactly the lanes below t of the current chunk and the lanes from t up of the previous
//                 one, so every lane evaluates its ONE candidate, selected by lane < t; neither LDS nor global memory holds the
//                 window.  The arg-max over (t(j, i), nearness of j) is one 64-bit key, (t << 6) | (64 - (i - j)), reduced by
//                 wave_max_u64_dpp (kmu_device.h: no LDS); 0 is "no predecessor beats a fresh start".  t < 2^32 * 64 + 64 < 2^39
//                 whatever the input (fewer than 2^32 anchors of at most 64 each), so the key never overflows; only candidates
//                 with t > span are keyed, so it is never negative.  Lane t keeps f, start and n; a wave-uniform running best (the
//                 first of the largest f) is the group's result.  A group of one anchor takes no step.
//  k_chain_best   COUNT and WRITE.  One lane per read pair over its one or two group results (s = 0 comes first and wins a tie),
//                 the min_score and min_seeds filters on the winner alone.  COUNT leaves a 0/1 per read pair, runs_total the
//                 offsets and the total, WRITE the records: ordered by (read_a, read_b) because the read pairs are.
//
// kmu_seed_chains_all reports EVERY chain of every group: the same anchors, keys, grouping and DP, then the decomposition of each
// group's forest of pred links into chains (the contract is in include/kmu.h).
//  k_chain_dp_all the ALL instance of k_chain_dp: lane t also keeps its chosen predecessor, and every chunk leaves f (8 bytes) and
//                 pred (4 bytes, CHAIN_NONE without one) per sorted anchor.  The group results (gf ..) are not written.
//  k_chain_sweep  one wave per group, no LDS, two sweeps over the chunks of 64 the DP used.  REVERSE, from the last chunk to the
//                 first, with the chunk below in registers as well: lane l holds the key (f, index) of the best end known for its
//                 anchor, at first its own.  Step t (descending) reads lane t's key and pred by readlane; every anchor above t has
//                 handed its key down by then, so the key is final, and the lane of pred(t) -- in this chunk, or in the one
//                 below, since pred(i) >= i - 64 -- keeps the better of the two (larger f, then the smaller index).  A finished
//                 chunk leaves best per anchor (4 bytes).  FORWARD, from the first chunk to the last with the chunk above it in
//                 registers: anchor t continues its predecessor's chain (count + 1, the same first member) iff both have the same
//                 best, otherwise it starts one.  An anchor that is its own best is an END; it leaves its count and first member,
//                 and the ends that pass the filters are counted per group (ballot), which is the group's keep word.
//  k_chain_all_write  one wave per group that keeps something: the reported ends in ascending order behind the group's offset,
//                 placed by ballot and prefix count.  Groups are ordered (read_a, read_b, s), so the records are.
// Both sweeps read lanes by a wave-uniform index (v_readlane) and reduce nothing; there is no atomic, no float and no LDS.
#include <algorithm>

#include "kmu_runs.h"

namespace kmu {

struct ChainArgs {
    PairRuns r;            // n_max = n_pairs: an anchor is an entry
    const uint32_t *pairs; // n_pairs x 2
    const uint32_t *pos_q, *read_q, *pos_db, *read_db;
    const uint8_t *strand_q, *strand_db; // or null
    uint32_t n_q, n_reads_q, n_db, n_reads_db;
    uint32_t span, max_gap, band, min_seeds, min_score, upper;
    uint32_t pos_lim; // the largest position the call takes
    uint32_t ybias;   // the low word of sec is y + ybias
    uint64_t *sec;    // per anchor c
    // per group: the best f, the sorted anchor that has it, that anchor's start and seed count
    uint64_t *gf;
    uint32_t *gend, *gbeg, *gn;
    kmu_chain *out;
    // kmu_seed_chains_all, per sorted anchor: f and the chosen predecessor (CHAIN_NONE: none), the end of its chain; per end:
    // the members of its chain and the first of them
    uint64_t *af;
    uint32_t *apred, *abest, *acnt, *afirst;
};

static constexpr uint32_t CHAIN_NONE = 0xFFFFFFFFu;

__device__ __forceinline__ uint32_t chain_x(uint64_t sec) { return (uint32_t) (sec >> 32) & 0x7FFFFFFFu; }
__device__ __forceinline__ int32_t chain_y(const ChainArgs &a, uint64_t sec) { return (int32_t) ((uint32_t) sec - a.ybias); }
// the position on the database side of a sorted anchor
__device__ __forceinline__ uint32_t chain_pos_db(const ChainArgs &a, uint64_t sec) {
    const int32_t y = chain_y(a, sec);
    return (uint32_t) ((sec >> 63) ? -y : y);
}

struct ChainPairs {
    struct Item {
        uint32_t ra, rb, x, pb, s;
    };
    static __device__ __forceinline__ bool decode(const ChainArgs &a, uint64_t p, Item &it, uint32_t &bad) {
        const uint32_t ea = a.pairs[2 * p], eb = a.pairs[2 * p + 1];
        bool refused = true;
        if (ea < a.n_q && eb < a.n_db) {
            it.ra = a.read_q[ea];
            it.rb = a.read_db[eb];
            it.x = a.pos_q[ea];
            it.pb = a.pos_db[eb];
            it.s = ((a.strand_q ? a.strand_q[ea] : 0u) ^ (a.strand_db ? a.strand_db[eb] : 0u)) & 1u;
            refused = it.ra >= a.n_reads_q || it.rb >= a.n_reads_db || it.x > a.pos_lim || it.pb > a.pos_lim;
        }
        if (refused) { // the call is refused at its synchronisation: until then the anchor only has to be harmless
            bad = 1;
            it = Item{};
        }
        return !a.upper || it.ra < it.rb;
    }
    static __device__ __forceinline__ void store(const ChainArgs &a, uint64_t, uint64_t c, const Item &it) {
        const uint32_t yb = (it.s ? 0u - it.pb : it.pb) + a.ybias;
        const uint64_t sec = ((uint64_t) it.s << 63) | ((uint64_t) it.x << 32) | yb;
        a.r.prim[c] = ((uint64_t) it.ra << 32) | it.rb;
        a.sec[c] = sec;
        a.r.skeys[c] = sec;
        a.r.svals[c] = (uint32_t) c;
    }
    static __device__ __forceinline__ uint64_t inner(const ChainArgs &a, uint32_t v) { return a.sec[v] >> 63; }
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_chain_keys(ChainArgs a) { runs_compact<ChainPairs, WRITE>(a); }

// ALL: kmu_seed_chains_all -- f and pred of every sorted anchor instead of the group's winner
template <bool ALL> __global__ void __launch_bounds__(64) k_chain_dp(ChainArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_groups = a.r.ridx[a.r.n_max];
    const int64_t span = a.span, max_gap = a.max_gap, band = a.band;
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t beg = a.r.rstart[g], end = a.r.rstart[g + 1];
        // anchor 0 of the group: f = span, a chain of its own.  Only a strictly larger f replaces it: the smallest i of the largest f
        uint64_t best_f = (uint64_t) span;
        uint32_t best_e = beg, best_b = beg, best_n = 1;
        if (ALL || end - beg > 1) { // uniform
            uint32_t px = 0, pb = 0, pn = 0; // the previous chunk
            int32_t py = 0;
            uint64_t pf = 0;
            for (uint64_t at = beg; at < end; at += 64) { // (64 bits: the last chunk may end within 64 of 2^32)
                const uint32_t c0 = (uint32_t) at;
                const uint32_t cnt = min(64u, end - c0);
                const bool has_prev = c0 > beg;
                uint32_t cx = 0, cb = c0 + lane, cn = 1;
                int32_t cy = 0;
                uint64_t cf = (uint64_t) span;
                uint32_t cpred = CHAIN_NONE; // (ALL)
                if (lane < cnt) {
                    const uint64_t sec = a.sec[a.r.svals[c0 + lane]];
                    cx = chain_x(sec);
                    cy = chain_y(a, sec);
                }
                for (uint32_t t = has_prev ? 0u : 1u; t < cnt; t++) { // t is wave-uniform
                    const int64_t xi = readlane_u32(cx, t), yi = (int32_t) readlane_u32((uint32_t) cy, t);
                    const bool own = lane < t; // the candidate is of this chunk: anchor c0 + lane; otherwise c0 - 64 + lane
                    const int64_t dx = xi - (int64_t) (own ? cx : px), dy = yi - (int64_t) (own ? cy : py);
                    const uint64_t jf = own ? cf : pf;
                    uint64_t key = 0;
                    if ((own || has_prev) && dx > 0 && dx <= max_gap && dy > 0 && dy <= max_gap) {
                        const int64_t d = dx - dy;
                        const uint64_t gg = (uint64_t) (d < 0 ? -d : d);
                        if ((int64_t) gg <= band) {
                            const uint64_t cost = gg ? ((gg * (uint64_t) span) >> 7) + ((63u - (uint32_t) __clzll((long long) gg)) >> 1) : 0ull;
                            const int64_t tv = (int64_t) jf + std::min(std::min(dx, dy), span) - (int64_t) cost;
                            // nearness 64 - (i - j): i - j = t - lane in this chunk, t - lane + 64 in the previous one
                            if (tv > span) key = ((uint64_t) tv << 6) | (63u - ((t - lane - 1u) & 63u));
                        }
                    }
                    key = wave_max_u64_dpp(key);
                    if (key) { // uniform
                        const uint32_t l = (t - 1u - (63u - ((uint32_t) key & 63u))) & 63u; // the lane of the chosen predecessor
                        const uint64_t fi = key >> 6;
                        const uint32_t bi = l < t ? readlane_u32(cb, l) : readlane_u32(pb, l);
                        const uint32_t ni = (l < t ? readlane_u32(cn, l) : readlane_u32(pn, l)) + 1u;
                        if (lane == t) {
                            cf = fi;
                            cb = bi;
                            cn = ni;
                            if (ALL) cpred = c0 + t - (64u - ((uint32_t) key & 63u)); // i - j = 64 - nearness
                        }
                        if (!ALL && fi > best_f) {
                            best_f = fi;
                            best_e = c0 + t;
                            best_b = bi;
                            best_n = ni;
                        }
                    }
                }
                if (ALL && lane < cnt) {
                    a.af[c0 + lane] = cf;
                    a.apred[c0 + lane] = cpred;
                }
                px = cx;
                py = cy;
                pf = cf;
                pb = cb;
                pn = cn;
            }
        }
        if (!ALL && lane == 0) {
            a.gf[g] = best_f;
            a.gend[g] = best_e;
            a.gbeg[g] = best_b;
            a.gn[g] = best_n;
        }
    }
}

template <bool WRITE> __global__ void __launch_bounds__(256) k_chain_best(ChainArgs a) {
    const uint64_t n_rp = a.r.pidx[a.r.n_max];
    for (uint64_t q = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; q < n_rp; q += (uint64_t) gridDim.x * blockDim.x) {
        if (WRITE && !a.r.keep[q]) continue;
        const uint32_t g0 = a.r.pstart[q], g1 = a.r.pstart[q + 1];
        uint32_t w = g0;
        for (uint32_t g = g0 + 1; g < g1; g++) // (one more at most: s = 1) the first of the largest stays
            if (a.gf[g] > a.gf[w]) w = g;
        const uint64_t f = a.gf[w];
        const uint32_t n = a.gn[w];
        if (!WRITE) {
            a.r.keep[q] = (f >= a.min_score && n >= a.min_seeds) ? 1u : 0u;
        } else {
            const uint64_t o = a.r.ooff[q];
            if (o < a.r.total) {
                const uint32_t e = a.gend[w], b = a.gbeg[w];
                const uint64_t rp = a.r.skeys[e], sec_e = a.sec[a.r.svals[e]], sec_b = a.sec[a.r.svals[b]];
                const uint32_t s = (uint32_t) (sec_e >> 63);
                kmu_chain rec;
                rec.read_a = (uint32_t) (rp >> 32);
                rec.read_b = (uint32_t) rp;
                rec.strand = s;
                rec.score = f > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) f;
                rec.n_seeds = n;
                rec.n_anchors = a.r.rstart[w + 1] - a.r.rstart[w];
                rec.a_start = chain_x(sec_b);
                rec.a_end = chain_x(sec_e) + a.span;
                rec.b_start = chain_pos_db(a, s ? sec_e : sec_b);
                rec.b_end = chain_pos_db(a, s ? sec_b : sec_e) + a.span;
                a.out[o] = rec;
            }
        }
    }
}

// ---- kmu_seed_chains_all: the chains of a group's forest ------------------------------------------------------------------------
// the 64 bits of lane l (wave-uniform l)
__device__ __forceinline__ uint64_t readlane_u64(uint64_t v, uint32_t l) {
    return ((uint64_t) readlane_u32((uint32_t) (v >> 32), l) << 32) | readlane_u32((uint32_t) v, l);
}

// The chain that ends in sorted anchor e, first member `first`, n members: its score, and whether it is reported.
// score = f(e) - f(p) with p = pred(first), f(e) without one; in 64 bits, clamped to 0 .. 2^32 - 1.
__device__ __forceinline__ bool chain_all_reported(const ChainArgs &a, uint32_t e, uint32_t first, uint32_t n, uint32_t &score) {
    const uint32_t p = a.apred[first];
    const int64_t s = (int64_t) a.af[e] - (p != CHAIN_NONE ? (int64_t) a.af[p] : 0ll);
    score = s < 0 ? 0u : s > 0xFFFFFFFFll ? 0xFFFFFFFFu : (uint32_t) s;
    return score >= a.min_score && n >= a.min_seeds;
}

__global__ void __launch_bounds__(64) k_chain_sweep(ChainArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_groups = a.r.ridx[a.r.n_max];
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t beg = a.r.rstart[g], end = a.r.rstart[g + 1];
        if (end <= beg) continue; // (uniform; a group has an anchor)
        const uint32_t n_chunks = (end - beg + 63u) >> 6; // chunk k is the anchors beg + 64 k .., as in the DP
        // REVERSE: the best end of every anchor.  (kf, kd): the key of this lane's anchor, kd the end, kf its f
        uint64_t ckf = 0, lkf = 0;
        uint32_t ckd = 0, lkd = 0, cp = CHAIN_NONE, lp = CHAIN_NONE;
        {
            const uint32_t c0 = beg + ((n_chunks - 1u) << 6);
            if (lane < end - c0) {
                ckf = a.af[c0 + lane];
                cp = a.apred[c0 + lane];
            }
            ckd = c0 + lane;
        }
        for (uint32_t k = n_chunks; k-- > 0;) { // uniform
            const uint32_t c0 = beg + (k << 6);
            const uint32_t cnt = min(64u, end - c0);
            if (k > 0) { // the chunk below is whole
                lkf = a.af[c0 - 64u + lane];
                lp = a.apred[c0 - 64u + lane];
                lkd = c0 - 64u + lane;
            }
            for (uint32_t t = cnt; t-- > 0;) {
                const uint32_t p = readlane_u32(cp, t);
                if (p == CHAIN_NONE) continue; // uniform
                const uint64_t kf = readlane_u64(ckf, t);
                const uint32_t kd = readlane_u32(ckd, t);
                if (lane == ((p - c0) & 63u)) { // p - c0 in this chunk, p - c0 + 64 in the one below
                    if (p >= c0) {
                        if (kf > ckf || (kf == ckf && kd < ckd)) {
                            ckf = kf;
                            ckd = kd;
                        }
                    } else if (kf > lkf || (kf == lkf && kd < lkd)) {
                        lkf = kf;
                        lkd = kd;
                    }
                }
            }
            if (lane < cnt) a.abest[c0 + lane] = ckd;
            ckf = lkf;
            ckd = lkd;
            cp = lp;
        }
        // FORWARD: count and first member of every chain so far; the ends; how many of them are reported
        uint32_t pbest = 0, pn = 0, pfirst = 0, kept = 0;
        for (uint32_t k = 0; k < n_chunks; k++) {
            const uint32_t c0 = beg + (k << 6);
            const uint32_t cnt = min(64u, end - c0);
            uint32_t cbest = CHAIN_NONE, cn = 1, cfirst = c0 + lane;
            cp = CHAIN_NONE;
            if (lane < cnt) {
                cbest = a.abest[c0 + lane]; // (this lane wrote it)
                cp = a.apred[c0 + lane];
            }
            for (uint32_t t = k ? 0u : 1u; t < cnt; t++) {
                const uint32_t p = readlane_u32(cp, t);
                if (p == CHAIN_NONE) continue; // uniform
                const uint32_t l = (p - c0) & 63u;
                const bool own = p >= c0;
                if ((own ? readlane_u32(cbest, l) : readlane_u32(pbest, l)) != readlane_u32(cbest, t)) continue;
                const uint32_t ni = (own ? readlane_u32(cn, l) : readlane_u32(pn, l)) + 1u;
                const uint32_t bi = own ? readlane_u32(cfirst, l) : readlane_u32(pfirst, l);
                if (lane == t) {
                    cn = ni;
                    cfirst = bi;
                }
            }
            bool rep = false;
            if (lane < cnt && cbest == c0 + lane) {
                uint32_t score;
                a.acnt[c0 + lane] = cn;
                a.afirst[c0 + lane] = cfirst;
                rep = chain_all_reported(a, c0 + lane, cfirst, cn, score);
            }
            kept += (uint32_t) __popcll(__ballot(rep));
            pbest = cbest;
            pn = cn;
            pfirst = cfirst;
        }
        if (lane == 0) a.r.keep[g] = kept;
    }
}

__global__ void __launch_bounds__(64) k_chain_all_write(ChainArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_groups = a.r.ridx[a.r.n_max];
    const uint64_t below = (1ull << lane) - 1ull;
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        if (!a.r.keep[g]) continue; // uniform
        const uint32_t beg = a.r.rstart[g], end = a.r.rstart[g + 1];
        uint64_t at = a.r.ooff[g];
        for (uint64_t c = beg; c < end; c += 64) { // (64 bits: the last chunk may end within 64 of 2^32)
            const uint32_t e = (uint32_t) c + lane;
            bool rep = false;
            uint32_t score = 0, n = 0, b = 0;
            if (lane < end - (uint32_t) c && a.abest[e] == e) {
                n = a.acnt[e];
                b = a.afirst[e];
                rep = chain_all_reported(a, e, b, n, score);
            }
            const uint64_t bal = __ballot(rep);
            const uint64_t o = at + (uint64_t) __popcll(bal & below);
            if (rep && o < a.r.total) {
                const uint64_t rp = a.r.skeys[e], sec_e = a.sec[a.r.svals[e]], sec_b = a.sec[a.r.svals[b]];
                const uint32_t s = (uint32_t) (sec_e >> 63);
                kmu_chain rec;
                rec.read_a = (uint32_t) (rp >> 32);
                rec.read_b = (uint32_t) rp;
                rec.strand = s;
                rec.score = score;
                rec.n_seeds = n;
                rec.n_anchors = end - beg;
                rec.a_start = chain_x(sec_b);
                rec.a_end = chain_x(sec_e) + a.span;
                rec.b_start = chain_pos_db(a, s ? sec_e : sec_b);
                rec.b_end = chain_pos_db(a, s ? sec_b : sec_e) + a.span;
                a.out[o] = rec;
            }
            at += (uint64_t) __popcll(bal);
        }
    }
}

} // namespace kmu

using namespace kmu;

// both entries: the arguments, the anchors and their groups are the same; `all` chooses what is made of a group
static int seed_chains_call(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs, const uint32_t *pos_q, const uint32_t *read_q,
                            const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q, const uint32_t *pos_db, const uint32_t *read_db,
                            const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db, const kmu_chain_params *p, int mem,
                            kmu_chain *out, uint64_t cap, uint64_t *n_out, bool all) {
    if (!ctx || !pairs || !pos_q || !read_q || !pos_db || !read_db || !p || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->span == 0 || p->span > 64) return fail(ctx, KMU_E_BAD_ARG, "span = %u: must be 1 .. 64", p->span);
    if (p->max_gap == 0) return fail(ctx, KMU_E_BAD_ARG, "max_gap = 0: no seed could follow another");
    if (p->min_seeds == 0) return fail(ctx, KMU_E_BAD_ARG, "min_seeds = 0: a chain has at least one seed");
    if (p->flags & ~KMU_CHAIN_UPPER) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags & ~KMU_CHAIN_UPPER);
    KMU_TRY(check_mem(ctx, mem));
    if (n_pairs > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu pairs: 2^32 or more", (unsigned long long) n_pairs);
    *n_out = 0;
    if (n_pairs == 0) return KMU_OK;
    if (n_q == 0 || n_db == 0 || n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "pairs but no entries or no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    ChainArgs a{};
    KMU_TRY(stage_to_device(ctx, "chain.pairs", pairs, (size_t) n_pairs * 2, mem, &a.pairs));
    KMU_TRY(stage_to_device(ctx, "chain.posq", pos_q, (size_t) n_q, mem, &a.pos_q));
    KMU_TRY(stage_to_device(ctx, "chain.readq", read_q, (size_t) n_q, mem, &a.read_q));
    KMU_TRY(stage_to_device(ctx, "chain.strandq", strand_q, (size_t) n_q, mem, &a.strand_q));
    if (pos_db == pos_q && read_db == read_q && strand_db == strand_q && n_db == n_q) { // a self-join is staged once
        a.pos_db = a.pos_q;
        a.read_db = a.read_q;
        a.strand_db = a.strand_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "chain.posdb", pos_db, (size_t) n_db, mem, &a.pos_db));
        KMU_TRY(stage_to_device(ctx, "chain.readdb", read_db, (size_t) n_db, mem, &a.read_db));
        KMU_TRY(stage_to_device(ctx, "chain.stranddb", strand_db, (size_t) n_db, mem, &a.strand_db));
    }
    a.n_q = n_q;
    a.n_reads_q = n_reads_q;
    a.n_db = n_db;
    a.n_reads_db = n_reads_db;
    a.span = p->span;
    a.max_gap = p->max_gap;
    a.band = p->band;
    a.min_seeds = p->min_seeds;
    a.min_score = p->min_score;
    a.upper = (p->flags & KMU_CHAIN_UPPER) ? 1u : 0u;
    a.pos_lim = p->max_pos ? std::min(p->max_pos, 0x7FFFFFFFu) : 0x7FFFFFFFu;
    a.ybias = p->max_pos ? a.pos_lim : 0x80000000u;

    char refusal[96];
    snprintf(refusal, sizeof refusal, "a pair names an entry or a read that does not exist, or a position above %u", a.pos_lim);

    KMU_TRY(runs_workspace(ctx, a.r, n_pairs, 1, 0, a.upper));
    KMU_TRY(dev_array(ctx, "chain.sec", n_pairs, &a.sec));
    if (!all) {
        KMU_TRY(dev_array(ctx, "chain.gf", n_pairs, &a.gf));
        KMU_TRY(dev_array(ctx, "chain.gend", n_pairs, &a.gend));
        KMU_TRY(dev_array(ctx, "chain.gbeg", n_pairs, &a.gbeg));
        KMU_TRY(dev_array(ctx, "chain.gn", n_pairs, &a.gn));
    } else {
        KMU_TRY(dev_array(ctx, "chain.af", n_pairs, &a.af));
        KMU_TRY(dev_array(ctx, "chain.apred", n_pairs, &a.apred));
        KMU_TRY(dev_array(ctx, "chain.abest", n_pairs, &a.abest));
        KMU_TRY(dev_array(ctx, "chain.acnt", n_pairs, &a.acnt));
        KMU_TRY(dev_array(ctx, "chain.afirst", n_pairs, &a.afirst));
    }

    // anchors; by (s, x, y), then (stable) by read pair: only the bytes that can differ; groups and read pairs
    KMU_TRY(runs_keys(ctx, "chain", a, k_chain_keys<false>, k_chain_keys<true>));
    const bool stranded = strand_q || strand_db;
    const uint32_t sec_passes =
        p->max_pos ? (radix_id_passes(2u * a.pos_lim + 1u) | (radix_id_passes(a.pos_lim + 1u) << 4) | (stranded ? 0x80u : 0u)) : 0xFFu;
    KMU_TRY(runs_order<ChainPairs>(ctx, "chain", a, sec_passes, n_reads_q, n_reads_db));
    const uint32_t waves = grid_for(ctx, n_pairs, 1, 16); // (one-wave workgroups)
    bool emit;
    if (all) { // DP with f and pred kept, both sweeps with COUNT, total, WRITE
        KMU_TRY(launch(ctx, "k_chain_dp_all", k_chain_dp<true>, dim3(waves), dim3(64), 0, a));
        KMU_TRY(launch(ctx, "k_chain_sweep", k_chain_sweep, dim3(waves), dim3(64), 0, a));
        const int rc = runs_total(ctx, a.r, mem, out != nullptr, cap, n_out, "chains", refusal, &emit);
        if (!emit) return rc;
        return runs_emit(ctx, a.r, mem, out, [&](kmu_chain *where) {
            a.out = where;
            return launch(ctx, "k_chain_all_write", k_chain_all_write, dim3(waves), dim3(64), 0, a);
        });
    }
    KMU_TRY(launch(ctx, "k_chain_dp", k_chain_dp<false>, dim3(waves), dim3(64), 0, a));

    // COUNT, total, WRITE
    const uint32_t flat = grid_for(ctx, n_pairs, 256);
    KMU_TRY(launch(ctx, "k_chain_best_count", k_chain_best<false>, dim3(flat), dim3(256), 0, a));
    const int rc = runs_total(ctx, a.r, mem, out != nullptr, cap, n_out, "chains", refusal, &emit);
    if (!emit) return rc;
    return runs_emit(ctx, a.r, mem, out, [&](kmu_chain *where) {
        a.out = where;
        return launch(ctx, "k_chain_best_write", k_chain_best<true>, dim3(flat), dim3(256), 0, a);
    });
}

extern "C" int kmu_seed_chains(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs, const uint32_t *pos_q, const uint32_t *read_q,
                               const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q, const uint32_t *pos_db,
                               const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                               const kmu_chain_params *p, int mem, kmu_chain *out, uint64_t cap, uint64_t *n_out) {
    return seed_chains_call(ctx, pairs, n_pairs, pos_q, read_q, strand_q, n_q, n_reads_q, pos_db, read_db, strand_db, n_db, n_reads_db, p,
                            mem, out, cap, n_out, false);
}

extern "C" int kmu_seed_chains_all(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs, const uint32_t *pos_q, const uint32_t *read_q,
                                   const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q, const uint32_t *pos_db,
                                   const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                                   const kmu_chain_params *p, int mem, kmu_chain *out, uint64_t cap, uint64_t *n_out) {
    return seed_chains_call(ctx, pairs, n_pairs, pos_q, read_q, strand_q, n_q, n_reads_q, pos_db, read_db, strand_db, n_db, n_reads_db, p,
                            mem, out, cap, n_out, true);
}

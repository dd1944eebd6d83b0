// kmu_seed_chains.hip -- from minimizer hits (pairs of minimizer entries that carry the same hash) to one colinear chain per read
// pair, at base resolution and on the device (kmu_seed_chains; the contract is in include/kmu.h).  A pair (ea, eb) is an ANCHOR of
// the read pair (read_q[ea], read_db[eb]) with relative strand s, x = pos_q[ea] and y = +-pos_db[eb]; the anchors of one
// (read_a, read_b, s) are a GROUP, ordered by (x, y).
//
//  k_chain_keys   COUNT and WRITE.  One wave per tile of SORT_TILE pairs, one lane per pair: the gather of the six values, the range
//                 checks (a pair that fails one is never used as an index; it raises ChainInfo::bad and the call is refused at its
//                 one synchronisation), the KMU_CHAIN_UPPER test, survivors compacted in lane order by ballot and prefix count
//                 (COUNT leaves one count per tile, device_scan_u32 the offsets; without the flag every pair survives and COUNT is
//                 not run).  Anchor c keeps prim = read_a << 32 | read_b and sec = s << 63 | x << 32 | (y + ybias); sec is the first
//                 sort key, c the value.  ybias is 2^31, or max_pos where the caller promises one: the keys then differ in fewer
//                 bytes.  The number of anchors stays on the device (ChainInfo::n).
//  sort           radix_sort_pairs_passes on sec, k_chain_gather puts prim in its place, radix_sort_pairs_passes on that: stable,
//                 so the order is (read_a, read_b, s, x, y).
//  k_chain_heads  one lane per sorted anchor: does the group change here, does the read pair change here.  device_scan_u32 numbers
//                 both; k_run_starts (kmu_runs.h, shared with kmu_anchor_overlaps.hip) writes the first anchor of every group and
//                 the first group of every read pair.
//  k_chain_dp     one wave per group, groups dealt grid-stride.  The wave takes the anchors 64 at a time: lane l holds anchor
//                 c * 64 + l of chunk c in registers (x, y, f, start, n), and the same five of chunk c - 1.  The lookback window of
//                 anchor i = c * 64 + t is exactly the lanes below t of the current chunk and the lanes from t up of the previous
//                 one, so every lane evaluates its ONE candidate, selected by lane < t; neither LDS nor global memory holds the
//                 window.  The arg-max over (t(j, i), nearness of j) is one 64-bit key, (t << 6) | (64 - (i - j)), reduced with DPP
//                 row shifts and broadcasts on both halves; 0 is "no predecessor beats a fresh start".  t < 2^32 * 64 + 64 < 2^39
//                 whatever the input (fewer than 2^32 anchors of at most 64 each), so the key never overflows; only candidates
//                 with t > span are keyed, so it is never negative.  Lane t keeps f, start and n; a wave-uniform running best (the
//                 first of the largest f) is the group's result.  A group of one anchor takes no step.
//  k_chain_best   COUNT and WRITE.  One lane per read pair over its one or two group results (s = 0 comes first and wins a tie),
//                 the min_score and min_seeds filters on the winner alone.  COUNT leaves a 0/1 per read pair, device_scan_u32 the
//                 offsets, WRITE the records: ordered by (read_a, read_b) because the read pairs are.
#include <algorithm>

#include "kmu_runs.h"
#include "kmu_sort.h"

namespace kmu {

struct ChainInfo {
    uint64_t n;   // anchors after KMU_CHAIN_UPPER
    uint32_t bad; // a pair outside what the call supports
    uint32_t pad;
};

struct ChainArgs {
    const uint32_t *pairs; // n_pairs x 2
    uint64_t n_pairs;
    const uint32_t *pos_q, *read_q, *pos_db, *read_db;
    const uint8_t *strand_q, *strand_db; // or null
    uint32_t n_q, n_reads_q, n_db, n_reads_db;
    uint32_t span, max_gap, band, min_seeds, min_score, upper;
    uint32_t pos_lim; // the largest position the call takes
    uint32_t ybias;   // the low word of sec is y + ybias
    ChainInfo *info;
    // per anchor c
    uint64_t *prim, *sec;
    // per anchor, sorted
    const uint64_t *skeys; // read pairs
    const uint32_t *svals; // anchor numbers c
    uint32_t *ghead, *phead, *keep;
    const uint64_t *gidx, *pidx; // exclusive scans of the flags; [n_pairs] = groups, read pairs
    uint32_t *gstart, *pstart;   // first anchor of group g (and n behind the last); first group of read pair q
    // per group: the best f, the sorted anchor that has it, that anchor's start and seed count
    uint64_t *gf;
    uint32_t *gend, *gbeg, *gn;
    // output
    const uint64_t *ooff; // exclusive scan of keep; [n_pairs] = records
    uint64_t total;
    kmu_chain *out;
};

__device__ __forceinline__ uint32_t chain_x(uint64_t sec) { return (uint32_t) (sec >> 32) & 0x7FFFFFFFu; }
__device__ __forceinline__ int32_t chain_y(const ChainArgs &a, uint64_t sec) { return (int32_t) ((uint32_t) sec - a.ybias); }
// the position on the database side of a sorted anchor
__device__ __forceinline__ uint32_t chain_pos_db(const ChainArgs &a, uint64_t sec) {
    const int32_t y = chain_y(a, sec);
    return (uint32_t) ((sec >> 63) ? -y : y);
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_chain_keys(ChainArgs a, uint32_t *counts, const uint64_t *coff,
                                                                          uint32_t n_tiles, uint64_t *keys, uint32_t *vals) {
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t t0 = (uint64_t) tile * SORT_TILE;
    uint64_t at = WRITE ? (coff ? coff[tile] : t0) : 0ull; // where the tile's next anchor goes / how many it keeps so far
    if (WRITE && tile == 0 && lane == 0) a.info->n = coff ? coff[n_tiles] : a.n_pairs;
    uint32_t bad = 0;
    for (uint32_t c0 = 0; c0 < SORT_TILE; c0 += 64) { // uniform trip count: all lanes reach the ballot
        const uint64_t p = t0 + c0 + lane;
        bool pass = p < a.n_pairs;
        uint32_t ra = 0, rb = 0, x = 0, pb = 0, s = 0;
        if (pass) {
            const uint32_t ea = a.pairs[2 * p], eb = a.pairs[2 * p + 1];
            bool refused = true;
            if (ea < a.n_q && eb < a.n_db) {
                ra = a.read_q[ea];
                rb = a.read_db[eb];
                x = a.pos_q[ea];
                pb = a.pos_db[eb];
                s = ((a.strand_q ? a.strand_q[ea] : 0u) ^ (a.strand_db ? a.strand_db[eb] : 0u)) & 1u;
                refused = ra >= a.n_reads_q || rb >= a.n_reads_db || x > a.pos_lim || pb > a.pos_lim;
            }
            if (refused) { // the call is refused at its synchronisation: until then the anchor only has to be harmless
                bad = 1;
                ra = rb = x = pb = s = 0;
            }
            pass = !a.upper || ra < rb;
        }
        const uint64_t bal = __ballot(pass);
        if (WRITE) {
            const uint64_t c = at + (uint64_t) __popcll(bal & below);
            if (pass && c < a.n_pairs) {
                const uint32_t yb = (s ? 0u - pb : pb) + a.ybias;
                const uint64_t sec = ((uint64_t) s << 63) | ((uint64_t) x << 32) | yb;
                a.prim[c] = ((uint64_t) ra << 32) | rb;
                a.sec[c] = sec;
                keys[c] = sec;
                vals[c] = (uint32_t) c;
            }
        }
        at += (uint64_t) __popcll(bal);
    }
    if (!WRITE && lane == 0) counts[tile] = (uint32_t) at;
    if (WRITE && bad) atomicOr(&a.info->bad, 1u);
}

// the read pair of every anchor, in the order the first sort left
__global__ void __launch_bounds__(256) k_chain_gather(ChainArgs a, const uint32_t *vals, uint64_t *keys) {
    const uint64_t n = min(a.info->n, a.n_pairs);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        keys[i] = a.prim[vals[i]];
}

// where a group begins and where a read pair begins; behind the last anchor the flags are 0, and so is every keep
__global__ void __launch_bounds__(256) k_chain_heads(ChainArgs a) {
    const uint64_t n = min(a.info->n, a.n_pairs);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_pairs; i += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t gh = 0, ph = 0;
        if (i < n) {
            ph = i == 0 || a.skeys[i] != a.skeys[i - 1];
            gh = ph || (a.sec[a.svals[i]] >> 63) != (a.sec[a.svals[i - 1]] >> 63);
        }
        a.ghead[i] = gh;
        a.phead[i] = ph;
        a.keep[i] = 0;
    }
}

// maximum of a 64-bit value over the 64 lanes, in every lane: the DPP steps of wave_max_u32 on both halves.  A lane that a step
// gives no source reads 0, which no maximum of unsigned values minds.  All lanes must be active.
#define KMU_CHAIN_DPP_MAX(ctrl, rows)                                                                        \
    do {                                                                                                     \
        const uint32_t oh_ = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (v >> 32), ctrl, rows, 0xf, false); \
        const uint32_t ol_ = (uint32_t) __builtin_amdgcn_update_dpp(0, (int) (uint32_t) v, ctrl, rows, 0xf, false); \
        const uint64_t o_ = ((uint64_t) oh_ << 32) | ol_;                                                    \
        v = o_ > v ? o_ : v;                                                                                 \
    } while (0)
__device__ __forceinline__ uint64_t chain_wave_max_u64(uint64_t v) {
    KMU_CHAIN_DPP_MAX(0x111, 0xf); // row_shr:1
    KMU_CHAIN_DPP_MAX(0x112, 0xf); // row_shr:2
    KMU_CHAIN_DPP_MAX(0x114, 0xf); // row_shr:4
    KMU_CHAIN_DPP_MAX(0x118, 0xf); // row_shr:8
    KMU_CHAIN_DPP_MAX(0x142, 0xa); // row_bcast:15
    KMU_CHAIN_DPP_MAX(0x143, 0xc); // row_bcast:31
    return ((uint64_t) (uint32_t) __builtin_amdgcn_readlane((int) (v >> 32), 63) << 32) |
           (uint32_t) __builtin_amdgcn_readlane((int) (uint32_t) v, 63);
}
#undef KMU_CHAIN_DPP_MAX

__device__ __forceinline__ uint32_t chain_readlane(uint32_t v, uint32_t l) { return (uint32_t) __builtin_amdgcn_readlane((int) v, (int) l); }

__global__ void __launch_bounds__(64) k_chain_dp(ChainArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_groups = a.gidx[a.n_pairs];
    const int64_t span = a.span, max_gap = a.max_gap, band = a.band;
    for (uint64_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        const uint32_t beg = a.gstart[g], end = a.gstart[g + 1];
        // anchor 0 of the group: f = span, a chain of its own.  Only a strictly larger f replaces it: the smallest i of the largest f
        uint64_t best_f = (uint64_t) span;
        uint32_t best_e = beg, best_b = beg, best_n = 1;
        if (end - beg > 1) { // uniform
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
                if (lane < cnt) {
                    const uint64_t sec = a.sec[a.svals[c0 + lane]];
                    cx = chain_x(sec);
                    cy = chain_y(a, sec);
                }
                for (uint32_t t = has_prev ? 0u : 1u; t < cnt; t++) { // t is wave-uniform
                    const int64_t xi = chain_readlane(cx, t), yi = (int32_t) chain_readlane((uint32_t) cy, t);
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
                    key = chain_wave_max_u64(key);
                    if (key) { // uniform
                        const uint32_t l = (t - 1u - (63u - ((uint32_t) key & 63u))) & 63u; // the lane of the chosen predecessor
                        const uint64_t fi = key >> 6;
                        const uint32_t bi = l < t ? chain_readlane(cb, l) : chain_readlane(pb, l);
                        const uint32_t ni = (l < t ? chain_readlane(cn, l) : chain_readlane(pn, l)) + 1u;
                        if (lane == t) {
                            cf = fi;
                            cb = bi;
                            cn = ni;
                        }
                        if (fi > best_f) {
                            best_f = fi;
                            best_e = c0 + t;
                            best_b = bi;
                            best_n = ni;
                        }
                    }
                }
                px = cx;
                py = cy;
                pf = cf;
                pb = cb;
                pn = cn;
            }
        }
        if (lane == 0) {
            a.gf[g] = best_f;
            a.gend[g] = best_e;
            a.gbeg[g] = best_b;
            a.gn[g] = best_n;
        }
    }
}

template <bool WRITE> __global__ void __launch_bounds__(256) k_chain_best(ChainArgs a) {
    const uint64_t n_rp = a.pidx[a.n_pairs];
    for (uint64_t q = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; q < n_rp; q += (uint64_t) gridDim.x * blockDim.x) {
        if (WRITE && !a.keep[q]) continue;
        const uint32_t g0 = a.pstart[q], g1 = a.pstart[q + 1];
        uint32_t w = g0;
        for (uint32_t g = g0 + 1; g < g1; g++) // (one more at most: s = 1) the first of the largest stays
            if (a.gf[g] > a.gf[w]) w = g;
        const uint64_t f = a.gf[w];
        const uint32_t n = a.gn[w];
        if (!WRITE) {
            a.keep[q] = (f >= a.min_score && n >= a.min_seeds) ? 1u : 0u;
        } else {
            const uint64_t o = a.ooff[q];
            if (o < a.total) {
                const uint32_t e = a.gend[w], b = a.gbeg[w];
                const uint64_t rp = a.skeys[e], sec_e = a.sec[a.svals[e]], sec_b = a.sec[a.svals[b]];
                const uint32_t s = (uint32_t) (sec_e >> 63);
                kmu_chain rec;
                rec.read_a = (uint32_t) (rp >> 32);
                rec.read_b = (uint32_t) rp;
                rec.strand = s;
                rec.score = f > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) f;
                rec.n_seeds = n;
                rec.n_anchors = a.gstart[w + 1] - a.gstart[w];
                rec.a_start = chain_x(sec_b);
                rec.a_end = chain_x(sec_e) + a.span;
                rec.b_start = chain_pos_db(a, s ? sec_e : sec_b);
                rec.b_end = chain_pos_db(a, s ? sec_b : sec_e) + a.span;
                a.out[o] = rec;
            }
        }
    }
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_seed_chains(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs, const uint32_t *pos_q, const uint32_t *read_q,
                               const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q, const uint32_t *pos_db,
                               const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                               const kmu_chain_params *p, int mem, kmu_chain *out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !pairs || !pos_q || !read_q || !pos_db || !read_db || !p || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->span == 0 || p->span > 64) return fail(ctx, KMU_E_BAD_ARG, "span = %u: must be 1 .. 64", p->span);
    if (p->max_gap == 0) return fail(ctx, KMU_E_BAD_ARG, "max_gap = 0: no seed could follow another");
    if (p->min_seeds == 0) return fail(ctx, KMU_E_BAD_ARG, "min_seeds = 0: a chain has at least one seed");
    if (p->flags & ~KMU_CHAIN_UPPER) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags & ~KMU_CHAIN_UPPER);
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    if (n_pairs > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu pairs: 2^32 or more", (unsigned long long) n_pairs);
    *n_out = 0;
    if (n_pairs == 0) return KMU_OK;
    if (n_q == 0 || n_db == 0 || n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "pairs but no entries or no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t n_tiles = (uint32_t) ((n_pairs + SORT_TILE - 1) / SORT_TILE);

    ChainArgs a{};
    const void *d;
    KMU_TRY(stage_to_device(ctx, "chain.pairs", pairs, (size_t) n_pairs * 8, mem, &d));
    a.pairs = (const uint32_t *) d;
    KMU_TRY(stage_to_device(ctx, "chain.posq", pos_q, (size_t) n_q * 4, mem, &d));
    a.pos_q = (const uint32_t *) d;
    KMU_TRY(stage_to_device(ctx, "chain.readq", read_q, (size_t) n_q * 4, mem, &d));
    a.read_q = (const uint32_t *) d;
    KMU_TRY(stage_to_device(ctx, "chain.strandq", strand_q, (size_t) n_q, mem, &d));
    a.strand_q = (const uint8_t *) d;
    if (pos_db == pos_q && read_db == read_q && strand_db == strand_q && n_db == n_q) { // a self-join is staged once
        a.pos_db = a.pos_q;
        a.read_db = a.read_q;
        a.strand_db = a.strand_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "chain.posdb", pos_db, (size_t) n_db * 4, mem, &d));
        a.pos_db = (const uint32_t *) d;
        KMU_TRY(stage_to_device(ctx, "chain.readdb", read_db, (size_t) n_db * 4, mem, &d));
        a.read_db = (const uint32_t *) d;
        KMU_TRY(stage_to_device(ctx, "chain.stranddb", strand_db, (size_t) n_db, mem, &d));
        a.strand_db = (const uint8_t *) d;
    }
    a.n_pairs = n_pairs;
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

    uint32_t *counts, *v0, *v1;
    uint64_t *coff, *k0, *k1, *gidx, *pidx, *ooff; // (the scans write what the kernels read through ChainArgs)
    KMU_TRY(dev_array(ctx, "chain.info", 1, &a.info));
    KMU_TRY(dev_array(ctx, "chain.counts", n_tiles, &counts));
    KMU_TRY(dev_array(ctx, "chain.coff", (size_t) n_tiles + 1, &coff));
    KMU_TRY(dev_array(ctx, "chain.prim", n_pairs, &a.prim));
    KMU_TRY(dev_array(ctx, "chain.sec", n_pairs, &a.sec));
    KMU_TRY(dev_array(ctx, "chain.keys0", n_pairs, &k0));
    KMU_TRY(dev_array(ctx, "chain.vals0", n_pairs, &v0));
    KMU_TRY(dev_array(ctx, "chain.keys1", n_pairs, &k1));
    KMU_TRY(dev_array(ctx, "chain.vals1", n_pairs, &v1));
    KMU_TRY(dev_array(ctx, "chain.ghead", n_pairs, &a.ghead));
    KMU_TRY(dev_array(ctx, "chain.phead", n_pairs, &a.phead));
    KMU_TRY(dev_array(ctx, "chain.keep", n_pairs, &a.keep));
    KMU_TRY(dev_array(ctx, "chain.gidx", (size_t) n_pairs + 1, &gidx));
    KMU_TRY(dev_array(ctx, "chain.pidx", (size_t) n_pairs + 1, &pidx));
    KMU_TRY(dev_array(ctx, "chain.ooff", (size_t) n_pairs + 1, &ooff));
    KMU_TRY(dev_array(ctx, "chain.gstart", (size_t) n_pairs + 1, &a.gstart));
    KMU_TRY(dev_array(ctx, "chain.pstart", (size_t) n_pairs + 1, &a.pstart));
    KMU_TRY(dev_array(ctx, "chain.gf", n_pairs, &a.gf));
    KMU_TRY(dev_array(ctx, "chain.gend", n_pairs, &a.gend));
    KMU_TRY(dev_array(ctx, "chain.gbeg", n_pairs, &a.gbeg));
    KMU_TRY(dev_array(ctx, "chain.gn", n_pairs, &a.gn));
    a.gidx = gidx;
    a.pidx = pidx;
    a.ooff = ooff;
    const uint64_t *n_dev = &a.info->n;

    // anchors
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, sizeof(ChainInfo), ctx->stream));
    if (a.upper) {
        KMU_TRY(launch(ctx, "k_chain_keys_count", k_chain_keys<false>, dim3(n_tiles), dim3(64), 0, a, counts, nullptr, n_tiles, k0, v0));
        KMU_TRY(device_scan_u32(ctx, counts, n_tiles, coff));
    }
    KMU_TRY(launch(ctx, "k_chain_keys_write", k_chain_keys<true>, dim3(n_tiles), dim3(64), 0, a, counts, a.upper ? coff : nullptr, n_tiles, k0, v0));

    // by (s, x, y), then (stable) by read pair; only the bytes that can differ
    const bool stranded = strand_q || strand_db;
    const uint32_t sec_passes =
        p->max_pos ? (radix_id_passes(2u * a.pos_lim + 1u) | (radix_id_passes(a.pos_lim + 1u) << 4) | (stranded ? 0x80u : 0u)) : 0xFFu;
    const uint32_t flat = grid_for(ctx, n_pairs, 256);
    KMU_TRY(radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n_pairs, sec_passes, n_dev));
    KMU_TRY(launch(ctx, "k_chain_gather", k_chain_gather, dim3(flat), dim3(256), 0, a, v0, k0));
    KMU_TRY(radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n_pairs, radix_id_passes(n_reads_db) | (radix_id_passes(n_reads_q) << 4), n_dev));
    a.skeys = k0;
    a.svals = v0;

    // groups and read pairs
    KMU_TRY(launch(ctx, "k_chain_heads", k_chain_heads, dim3(flat), dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.ghead, n_pairs, gidx));
    KMU_TRY(device_scan_u32(ctx, a.phead, n_pairs, pidx));
    KMU_TRY(launch(ctx, "k_chain_starts", k_run_starts, dim3(flat), dim3(256), 0,
                   RunMarks{n_dev, n_pairs, a.ghead, a.phead, gidx, pidx, a.gstart, a.pstart}));
    KMU_TRY(launch(ctx, "k_chain_dp", k_chain_dp, dim3(grid_for(ctx, n_pairs, 1, 16)), dim3(64), 0, a)); // (one-wave workgroups)

    // COUNT, offsets, total
    KMU_TRY(launch(ctx, "k_chain_best_count", k_chain_best<false>, dim3(flat), dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.keep, n_pairs, ooff));
    uint64_t total = 0;
    ChainInfo h_info{};
    KMU_HIP(ctx, hipMemcpyAsync(&total, ooff + n_pairs, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(&h_info, a.info, sizeof h_info, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_info.bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED, "a pair names an entry or a read that does not exist, or a position above %u", a.pos_lim);
    }
    *n_out = total;
    if (!out || total == 0) return finish_call(ctx, mem);
    if (cap < total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu chains, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.total = total;
    a.out = out;
    if (mem == KMU_MEM_HOST) KMU_TRY(dev_array(ctx, "chain.out", total, &a.out));
    KMU_TRY(launch(ctx, "k_chain_best_write", k_chain_best<true>, dim3(flat), dim3(256), 0, a));
    if (mem == KMU_MEM_HOST) KMU_HIP(ctx, hipMemcpyAsync(out, a.out, total * sizeof(kmu_chain), hipMemcpyDeviceToHost, ctx->stream));
    return finish_call(ctx, mem);
}

// kmu_chain_rank.hip -- which chains of a query read are primary and which are secondary to one, on the device (kmu_chain_rank; the
// contract is in include/kmu.h).  The chains of one read_a are consecutive in the input and read_a does not fall.
//
//  k_rank_keys    one lane per chain c: the checks (read_a below n_reads_q, a_start <= a_end, read_a not below that of c - 1; a
//                 record that fails one raises bad, gets the harmless key of read 0 and is never used as an index) and the key
//                 read_a << 32 | ~score with the value c.  The stable sort of kmu_sort.h leaves every read's chains in rank order:
//                 score descending, then input index.  Only the bytes that can differ are sorted: the four of ~score and those
//                 n_reads_q reaches.
//  k_rank_starts  one lane per query read r (and one behind the last): the first sorted chain of a read >= r, by binary search --
//                 a read without chains has an empty range.
//  k_rank_walk    one wave per query read, reads dealt grid-stride, no LDS.  The wave takes the read's chains 64 at a time into
//                 its lanes and walks them in rank order (readlane).  The primaries found so far live in the lanes as well: the
//                 latest up to 64 in registers (lane l holds primary 64 j + l of the read: a_start, a_end, input index, n_sub,
//                 sub_score); a full set of 64 goes to the read's own slots of five workspace arrays, which lane l alone writes
//                 and reads again.  A chain is tested against the earlier primaries 64 at a time, oldest set first; a ballot
//                 finds the best-ranked hit, and the lane that holds it counts the secondary (the first one has the largest score).
//                 A chain without a hit becomes the next primary.  Rank and parent of a chain are written when it is walked,
//                 sub_score and n_sub of the primaries when the read is done.  The test is integer compares and one 64-bit product
//                 on each side.  A read of c chains costs c^2 / 64 lane-parallel tests in the worst case (all primary), sequential
//                 in one wave: the accepted limit, fine for tens to hundreds of chains per read.
#include "kmu_sort.h"

namespace kmu {

struct RankArgs {
    const kmu_chain *chains;
    uint64_t n;
    uint32_t n_reads_q, mask;
    uint32_t *bad;
    uint64_t *keys, *keys1;
    uint32_t *vals, *vals1;
    uint32_t *rstart;                   // n_reads_q + 1
    uint32_t *ws, *we, *wi, *wn, *wsub; // the primaries of a read that left the registers, in the read's slots
    kmu_chain_rank_rec *out;
};

__global__ void __launch_bounds__(256) k_rank_keys(RankArgs a) {
    uint32_t bad = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c < a.n; c += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_chain &r = a.chains[c];
        uint32_t ra = r.read_a, score = r.score;
        if (ra >= a.n_reads_q || r.a_start > r.a_end || (c > 0 && a.chains[c - 1].read_a > ra)) {
            bad = 1;
            ra = 0;
        }
        a.keys[c] = ((uint64_t) ra << 32) | (uint32_t) ~score;
        a.vals[c] = (uint32_t) c;
    }
    if (bad) atomicOr(a.bad, 1u);
}

__global__ void __launch_bounds__(256) k_rank_starts(RankArgs a) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r <= a.n_reads_q; r += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t lo = 0, hi = a.n; // the first sorted chain whose read is >= r
        while (lo < hi) {
            const uint64_t mid = (lo + hi) >> 1;
            if ((a.keys[mid] >> 32) < r) lo = mid + 1;
            else hi = mid;
        }
        a.rstart[r] = (uint32_t) lo;
    }
}

// is the chain [cs, ce) secondary to the primary [ps, pe)
__device__ __forceinline__ bool rank_masks(uint32_t mask, uint32_t cs, uint32_t ce, uint32_t ps, uint32_t pe) {
    const uint32_t lo = max(cs, ps), hi = min(ce, pe);
    if (hi <= lo) return false;
    return (uint64_t) (hi - lo) * 1000ull >= (uint64_t) mask * (uint64_t) min(ce - cs, pe - ps);
}

__global__ void __launch_bounds__(64) k_rank_walk(RankArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    for (uint32_t r = blockIdx.x; r < a.n_reads_q; r += gridDim.x) {
        const uint32_t beg = a.rstart[r], end = a.rstart[r + 1];
        uint32_t n_prim = 0;                               // uniform
        uint32_t ps = 0, pe = 0, pi = 0, pn = 0, psub = 0; // primary (n_prim & ~63) + lane, where lane < (n_prim & 63)
        for (uint64_t at = beg; at < end; at += 64) {      // (64 bits: the last chunk may end within 64 of 2^32)
            const uint32_t c0 = (uint32_t) at;
            const uint32_t cnt = min(64u, end - c0);
            uint32_t ci = 0, cs = 0, ce = 0, csc = 0;
            if (lane < cnt) {
                ci = a.vals[c0 + lane];
                const kmu_chain &rec = a.chains[ci];
                cs = rec.a_start;
                ce = rec.a_end;
                csc = rec.score;
            }
            for (uint32_t t = 0; t < cnt; t++) {
                const uint32_t xi = readlane_u32(ci, t), xs = readlane_u32(cs, t), xe = readlane_u32(ce, t), xsc = readlane_u32(csc, t);
                uint32_t parent = xi;
                bool found = false; // uniform
                const uint32_t full = n_prim & ~63u;
                for (uint32_t j = 0; j < full && !found; j += 64) { // the sets that left the registers, oldest first
                    const uint32_t slot = beg + j + lane;
                    const uint64_t hit = __ballot(rank_masks(a.mask, xs, xe, a.ws[slot], a.we[slot]));
                    if (hit) {
                        const uint32_t l = (uint32_t) __ffsll((long long) hit) - 1u;
                        if (lane == l) {
                            const uint32_t ns = a.wn[slot];
                            if (ns == 0) a.wsub[slot] = xsc;
                            a.wn[slot] = ns + 1u;
                        }
                        parent = readlane_u32(a.wi[slot], l); // (every lane reads its own slot)
                        found = true;
                    }
                }
                if (!found) {
                    const uint64_t hit = __ballot(lane < (n_prim & 63u) && rank_masks(a.mask, xs, xe, ps, pe));
                    if (hit) {
                        const uint32_t l = (uint32_t) __ffsll((long long) hit) - 1u;
                        if (lane == l) {
                            if (pn == 0) psub = xsc;
                            pn++;
                        }
                        parent = readlane_u32(pi, l);
                        found = true;
                    }
                }
                if (!found) { // the next primary
                    if (lane == (n_prim & 63u)) {
                        ps = xs;
                        pe = xe;
                        pi = xi;
                        pn = 0;
                        psub = 0;
                    }
                    n_prim++;
                    if ((n_prim & 63u) == 0) { // the registers are full: to the read's slots
                        const uint32_t slot = beg + n_prim - 64u + lane;
                        a.ws[slot] = ps;
                        a.we[slot] = pe;
                        a.wi[slot] = pi;
                        a.wn[slot] = pn;
                        a.wsub[slot] = psub;
                    }
                }
                if (lane == 0) {
                    a.out[xi].rank = c0 + t - beg;
                    a.out[xi].parent = parent;
                    if (found) {
                        a.out[xi].sub_score = 0;
                        a.out[xi].n_sub = 0;
                    }
                }
            }
        }
        // the primaries' secondaries
        for (uint32_t j = 0; j < (n_prim & ~63u); j += 64) {
            const uint32_t slot = beg + j + lane;
            const uint32_t idx = a.wi[slot];
            a.out[idx].sub_score = a.wsub[slot];
            a.out[idx].n_sub = a.wn[slot];
        }
        if (lane < (n_prim & 63u)) {
            a.out[pi].sub_score = psub;
            a.out[pi].n_sub = pn;
        }
    }
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_chain_rank(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, uint32_t n_reads_q, const kmu_rank_params *p,
                              int mem, kmu_chain_rank_rec *out) {
    if (!ctx || !chains || !p || !out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    if (p->mask_permille > 1000) return fail(ctx, KMU_E_BAD_ARG, "mask_permille = %u: above 1000", p->mask_permille);
    KMU_TRY(check_mem(ctx, mem));
    if (n_chains == 0) return KMU_OK;
    if (n_reads_q == 0) return fail(ctx, KMU_E_BAD_ARG, "chains but no reads");
    if (n_chains > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu chains: 2^32 or more", (unsigned long long) n_chains);
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    RankArgs a{};
    KMU_TRY(stage_to_device(ctx, "rank.chains", chains, (size_t) n_chains, mem, &a.chains));
    a.n = n_chains;
    a.n_reads_q = n_reads_q;
    a.mask = p->mask_permille;
    KMU_TRY(dev_array(ctx, "rank.bad", 1, &a.bad));
    KMU_HIP(ctx, hipMemsetAsync(a.bad, 0, sizeof(uint32_t), ctx->stream));
    KMU_TRY(dev_array(ctx, "rank.keys0", n_chains, &a.keys));
    KMU_TRY(dev_array(ctx, "rank.keys1", n_chains, &a.keys1));
    KMU_TRY(dev_array(ctx, "rank.vals0", n_chains, &a.vals));
    KMU_TRY(dev_array(ctx, "rank.vals1", n_chains, &a.vals1));
    KMU_TRY(dev_array(ctx, "rank.rstart", (size_t) n_reads_q + 1, &a.rstart));
    KMU_TRY(dev_array(ctx, "rank.ws", n_chains, &a.ws));
    KMU_TRY(dev_array(ctx, "rank.we", n_chains, &a.we));
    KMU_TRY(dev_array(ctx, "rank.wi", n_chains, &a.wi));
    KMU_TRY(dev_array(ctx, "rank.wn", n_chains, &a.wn));
    KMU_TRY(dev_array(ctx, "rank.wsub", n_chains, &a.wsub));
    KMU_TRY(place_output(ctx, "rank.out", out, n_chains, mem, &a.out));

    KMU_TRY(launch(ctx, "k_rank_keys", k_rank_keys, dim3(grid_for(ctx, n_chains, 256)), dim3(256), 0, a));
    KMU_TRY(radix_sort_pairs_passes(ctx, a.keys, a.vals, a.keys1, a.vals1, n_chains, 0x0Fu | (radix_id_passes(n_reads_q) << 4), nullptr));
    KMU_TRY(launch(ctx, "k_rank_starts", k_rank_starts, dim3(grid_for(ctx, (uint64_t) n_reads_q + 1, 256)), dim3(256), 0, a));
    KMU_TRY(launch(ctx, "k_rank_walk", k_rank_walk, dim3(grid_for(ctx, n_reads_q, 1, 16)), dim3(64), 0, a)); // (one-wave workgroups)
    uint32_t h_bad = 0;
    KMU_TRY(bring_output(ctx, out, a.out, n_chains, mem));
    KMU_TRY(read_back(ctx, {{&h_bad, a.bad}}));
    KMU_TRY(finish_synced(ctx));
    if (h_bad)
        return fail(ctx, KMU_E_UNSUPPORTED, "a chain names a query read that does not exist or has a start behind its end, or the chains "
                                            "of one read_a are not consecutive with read_a ascending");
    return KMU_OK;
}

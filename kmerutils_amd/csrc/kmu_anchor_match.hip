// kmu_anchor_match.hip -- pair bottom-k rows that share one of their smallest hashes (kmu_anchor_match): the join behind the
// reference's inverse index smallest hash -> (readnum, slicepos) (redis_dump, src/anchor.rs:187-197) with mininvhash_distance
// (src/sketching/minhash.rs:295-340) on every pair it finds, without leaving the device.  The match kernel and its driver live
// here, for this call and for the anchor index (kmu_anchor_index.hip) alike.
//
//  anchor_db_build   kmu_anchor_index.hip: the database's (key, row) entries sorted by key and a directory of the distinct keys,
//                    in the workspace.  kmu_anchor_match is "a directory in the workspace, matched once, forgotten".
//  k_anchor_match    instantiated twice, COUNT and WRITE, so that both passes walk identically.  One wave (a 64-thread
//                    workgroup) per query row, rows dealt grid-stride, the row in LDS.  Its keys are looked up one lane per key
//                    -- one binary search in the distinct keys -- and bucket begin, end and "masked" (max_occ > 0 and occupancy >
//                    max_occ; kmu_anchor_match passes 0: nothing is) wait in LDS next to the row.  A masked key is skipped
//                    without touching its bucket; the others, in ascending order, are walked 64 entries at a time, one lane per
//                    candidate (anchor_candidates): group test, "is this key the smallest unmasked hash the two rows share" (a
//                    merge of the two rows up to the key), the walk of k_minhash_distance (minhash_walk, kmu_device.h), the
//                    min_common filter; survivors are compacted in lane order with a ballot and a prefix count.
//  anchor_match_run  COUNT leaves one count per query row; device_scan_u32 turns the counts into u64 offsets; the total crosses
//                    to the host; WRITE puts every pair at its offset.  Output order: query row, key, database row.
//  One wave owns a whole bucket: a key shared by very many rows (low-complexity windows) is walked by 64 lanes and gives
//  quadratic output; the repeat mask is the anchor index's max_occ.
#include <algorithm>

#include "kmu_anchor_db.h"
#include "kmu_device.h"

namespace kmu {

static constexpr uint64_t PADDING = 0xFFFFFFFFFFFFFFFFull;

// One chunk of a bucket, by one whole wave: lane l has candidate entry e = chunk + l of the bucket that ends at `end` (lanes
// behind the end stand by: every lane reaches the ballot).  `row` is query row r (n1 entries, group g) and row[kk] the key of
// the bucket.  Group test; "is row[kk] the smallest hash under which the pair is seeded" -- a merge of the two rows up to the
// key: a common hash in front of it is a smaller shared key and the pair is reported there, unless `masked` says that this key
// of the query is masked: then it seeds nothing and is stepped over --; the walk of k_minhash_distance over the whole rows; the
// min_common filter.  Survivors are compacted in lane order with a ballot and a prefix count behind `at`, which moves on by
// their number (COUNT: only that).
template <bool WRITE>
__device__ __forceinline__ void anchor_candidates(const MatchArgs &a, const uint64_t *row, uint32_t n1, uint32_t r, uint32_t g,
                                                  uint32_t kk, const uint8_t *masked, uint32_t e, uint32_t end, uint64_t &at) {
    const uint32_t m = a.db.m;
    bool pass = e < end;
    uint32_t b = 0, d[3] = {0, 0, 0};
    if (pass) {
        b = a.db.srows[e];
        pass = b < a.db.ndb; // (always: an entry names a row of the database)
        if (pass && a.db.groups) pass = a.db.groups[b] != g;
    }
    if (pass) {
        const uint64_t *rb = a.db.rows + (uint64_t) b * m;
        // none in front of row[kk] (rb holds row[kk], so with ascending rows j stays in range; the bound keeps a malformed row
        // from running on)
        uint32_t i = 0, j = 0;
        while (i < kk && j < m) {
            const uint64_t x = row[i], y = rb[j];
            if (x == y) {
                if (!masked[i]) break;
                i++;
                j++;
            } else if (x < y) i++;
            else j++;
        }
        pass = i == kk;
        if (pass) {
            minhash_walk(row, n1, rb, bottomk_row_len(rb, m), d);
            pass = d[0] >= a.min_common;
        }
    }
    const uint64_t bal = __ballot(pass);
    if (WRITE) {
        const uint64_t o = at + (uint64_t) __popcll(bal & ((1ull << lane_id()) - 1ull));
        if (pass && o < a.total) {
            a.pairs[2 * o] = r;
            a.pairs[2 * o + 1] = b;
            if (a.dist) {
                a.dist[3 * o] = d[0];
                a.dist[3 * o + 1] = d[1];
                a.dist[3 * o + 2] = d[2];
            }
        }
    }
    at += (uint64_t) __popcll(bal);
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_anchor_match(MatchArgs a) {
    __shared__ uint64_t row[KMU_ANCHOR_MAX_NBKMER];
    __shared__ uint32_t kbeg[KMU_ANCHOR_MAX_NBKMER], kend[KMU_ANCHOR_MAX_NBKMER]; // the bucket of every key of the row
    __shared__ uint8_t kmask[KMU_ANCHOR_MAX_NBKMER];                              // 1: the key is masked
    const uint32_t lane = (uint32_t) lane_id(), m = a.db.m;
    const uint32_t n_distinct = *a.db.n_distinct;
    for (uint32_t r = blockIdx.x; r < a.nq; r += gridDim.x) {
        uint32_t n1 = 0;
        for (uint32_t t0 = 0; t0 < m; t0 += 64) { // uniform trip count
            const uint32_t t = t0 + lane;
            const uint64_t h = t < m ? a.q[(uint64_t) r * m + t] : PADDING;
            if (t < m) row[t] = h;
            n1 += (uint32_t) __popcll(__ballot(h != PADDING));
        }
        __syncthreads();
        const uint32_t nk = min(a.db.n_keys, n1);
        for (uint32_t t = lane; t < nk; t += 64) { // one lane per key
            const uint64_t key = row[t];
            uint32_t lo = 0, hi = n_distinct;
            while (lo < hi) { // first distinct key >= key
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.db.ukeys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            uint32_t beg = 0, end = 0; // a key the directory does not have, or an empty directory: an empty bucket
            if (lo < n_distinct && a.db.ukeys[lo] == key) {
                beg = a.db.ubeg[lo];
                end = a.db.ubeg[lo + 1];
            }
            kbeg[t] = beg;
            kend[t] = end;
            kmask[t] = a.max_occ > 0 && end - beg > a.max_occ;
        }
        __syncthreads();
        const uint32_t g = a.gq ? a.gq[r] : 0u;
        uint64_t at = WRITE ? a.offs[r] : 0ull; // where the next pair of this row goes / how many it has so far
        for (uint32_t kk = 0; kk < nk; kk++) {
            if (kmask[kk]) continue; // (the same byte in every lane)
            const uint32_t end = kend[kk];
            for (uint32_t c = kbeg[kk]; c < end; c += 64) // uniform: all lanes reach the ballot
                anchor_candidates<WRITE>(a, row, n1, r, g, kk, kmask, c + lane, end, at);
        }
        if (!WRITE && lane == 0) a.counts[r] = (uint32_t) at;
        __syncthreads(); // the next row overwrites the LDS copies
    }
}

int anchor_match_run(kmu_ctx *ctx, MatchArgs &a, uint32_t nq, int mem, uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap,
                     uint64_t *n_out) {
    // COUNT, offsets, total
    uint64_t *offs;
    uint32_t *counts;
    KMU_TRY(dev_array(ctx, "am.counts", (size_t) nq, &counts));
    KMU_TRY(dev_array(ctx, "am.offs", (size_t) nq + 1, &offs));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(nq, (uint64_t) ctx->num_cus * 32);
    a.nq = nq;
    a.counts = counts;
    KMU_TRY(launch(ctx, "k_anchor_match_count", k_anchor_match<false>, dim3(grid), dim3(64), 0, a));
    KMU_TRY(device_scan_u32(ctx, counts, nq, offs));
    uint64_t total = 0;
    KMU_TRY(read_back(ctx, {{&total, offs + nq}}));
    *n_out = total;
    if (!pairs_out || total == 0) return finish_call(ctx, mem);
    if (cap < total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu pairs, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.offs = offs;
    a.total = total;
    KMU_TRY(place_output(ctx, "am.pairs", pairs_out, total * 2, mem, &a.pairs));
    KMU_TRY(place_output(ctx, "am.dist", dist_out, total * 3, mem, &a.dist));
    KMU_TRY(launch(ctx, "k_anchor_match_write", k_anchor_match<true>, dim3(grid), dim3(64), 0, a));
    KMU_TRY(bring_output(ctx, pairs_out, a.pairs, total * 2, mem));
    KMU_TRY(bring_output(ctx, dist_out, a.dist, total * 3, mem));
    return finish_call(ctx, mem);
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_anchor_match(kmu_ctx *ctx, const uint64_t *hashes_q, uint32_t nq, const uint64_t *hashes_db, uint32_t ndb, uint32_t m,
                                uint32_t n_keys, uint32_t min_common, const uint32_t *group_q, const uint32_t *group_db, int mem,
                                uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !hashes_q || !hashes_db || !n_out || m == 0) return fail(ctx, KMU_E_BAD_ARG, "null argument or m == 0");
    if (n_keys == 0 || n_keys > m) return fail(ctx, KMU_E_BAD_ARG, "n_keys = %u: must be 1 .. m = %u", n_keys, m);
    if ((group_q == nullptr) != (group_db == nullptr))
        return fail(ctx, KMU_E_BAD_ARG, "group_q and group_db go together: both null or both given");
    KMU_TRY(check_mem(ctx, mem));
    if (m > KMU_ANCHOR_MAX_NBKMER) return fail(ctx, KMU_E_UNSUPPORTED, "m = %u above KMU_ANCHOR_MAX_NBKMER (%d)", m, KMU_ANCHOR_MAX_NBKMER);
    if ((uint64_t) ndb * n_keys > 0xFFFFFFFFull)
        return fail(ctx, KMU_E_UNSUPPORTED, "%u rows x %u keys: 2^32 index entries or more", ndb, n_keys);
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0 || ndb == 0) return KMU_OK;

    MatchArgs a{};
    KMU_TRY(stage_to_device(ctx, "am.q", hashes_q, (size_t) nq * m, mem, &a.q));
    if (hashes_db == hashes_q && ndb == nq) a.db.rows = a.q; // a self-join is staged once
    else {
        KMU_TRY(stage_to_device(ctx, "am.db", hashes_db, (size_t) ndb * m, mem, &a.db.rows));
    }
    if (group_q) {
        KMU_TRY(stage_to_device(ctx, "am.gq", group_q, (size_t) nq, mem, &a.gq));
        KMU_TRY(stage_to_device(ctx, "am.gdb", group_db, (size_t) ndb, mem, &a.db.groups));
    }
    a.db.ndb = ndb;
    a.db.m = m;
    a.db.n_keys = n_keys;
    a.min_common = min_common; // (max_occ stays 0: no mask)
    KMU_TRY(anchor_db_build(ctx, &a.db, nullptr));
    return anchor_match_run(ctx, a, nq, mem, pairs_out, dist_out, cap, n_out);
}

// kmu_anchor_match.hip -- pair bottom-k rows that share one of their smallest hashes (kmu_anchor_match): the join behind the
// reference's inverse index smallest hash -> (readnum, slicepos) (redis_dump, src/anchor.rs:187-197) with mininvhash_distance
// (src/sketching/minhash.rs:295-340) on every pair it finds, without leaving the device.
//
//  k_anchor_entries  (kmu_anchor_cand.h) the index: entry e = row * n_keys + t is (db[row][t], row), in row order.  The padding of
//                    a short row comes along as key u64::MAX: it sorts to the end and no query asks for it.
//  radix_sort_pairs  kmu_sort.h: the entries by key, stable -- ascending rows inside a key, which the output order rests on.
//  k_anchor_match    instantiated twice, COUNT and WRITE, so that both passes walk identically.  One wave (a 64-thread
//                    workgroup) per query row, rows dealt grid-stride, the row in LDS.  For each of its keys, in ascending order:
//                    lower and upper bound in the sorted keys, then the bucket 64 entries at a time, one lane per candidate:
//                    group test, "is this key the smallest hash the two rows share" (a merge of the two rows up to the key: a
//                    smaller common hash is a smaller shared key, and the pair is reported there), the walk of
//                    k_minhash_distance (minhash_walk, kmu_device.h), the min_common filter.  Survivors are compacted in lane
//                    order with a ballot and a prefix count (anchor_candidates, kmu_anchor_cand.h, which the anchor index shares).  COUNT leaves one count per query row; device_scan_u32 turns the
//                    counts into u64 offsets; WRITE puts every pair at its offset.  Output order: query row, key, database row.
//  One wave owns a whole bucket: a key shared by very many rows (low-complexity windows) is walked by 64 lanes and gives
//  quadratic output; the repeat mask lives in the anchor index (kmu_anchor_index.hip).
#include <algorithm>

#include "kmu_anchor_cand.h"
#include "kmu_sort.h"

namespace kmu {

struct MatchArgs {
    const uint64_t *q; // nq x m
    uint32_t nq, n_keys;
    const uint32_t *gq;    // with c.gdb: both or neither
    const uint64_t *skeys; // n_entries sorted keys (c.srows: their rows)
    uint32_t n_entries;
    uint32_t *counts;     // COUNT: pairs of every query row
    const uint64_t *offs; // WRITE: nq + 1 offsets, offs[nq] = total
    CandArgs c;
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_anchor_match(MatchArgs a) {
    __shared__ uint64_t row[KMU_ANCHOR_MAX_NBKMER];
    const uint32_t lane = (uint32_t) lane_id(), m = a.c.m;
    for (uint32_t r = blockIdx.x; r < a.nq; r += gridDim.x) {
        uint32_t n1 = 0;
        for (uint32_t t0 = 0; t0 < m; t0 += 64) { // uniform trip count
            const uint32_t t = t0 + lane;
            const uint64_t h = t < m ? a.q[(uint64_t) r * m + t] : 0xFFFFFFFFFFFFFFFFull;
            if (t < m) row[t] = h;
            n1 += (uint32_t) __popcll(__ballot(h != 0xFFFFFFFFFFFFFFFFull));
        }
        __syncthreads();
        const uint32_t nk = min(a.n_keys, n1);
        const uint32_t g = a.gq ? a.gq[r] : 0u;
        uint64_t at = WRITE ? a.offs[r] : 0ull; // where the next pair of this row goes / how many it has so far
        for (uint32_t kk = 0; kk < nk; kk++) {
            const uint64_t key = row[kk];
            uint32_t lo = 0, hi = a.n_entries;
            while (lo < hi) { // first entry with skeys >= key
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.skeys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t beg = lo;
            hi = a.n_entries;
            while (lo < hi) { // first entry with skeys > key
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.skeys[mid] <= key) lo = mid + 1;
                else hi = mid;
            }
            const uint32_t end = lo;
            for (uint32_t c = beg; c < end; c += 64) // uniform: all lanes reach the ballot
                anchor_candidates<WRITE>(a.c, row, n1, r, g, kk, nullptr, c + lane, end, at);
        }
        if (!WRITE && lane == 0) a.counts[r] = (uint32_t) at;
        __syncthreads(); // the next row overwrites the LDS copy
    }
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
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    if (m > KMU_ANCHOR_MAX_NBKMER) return fail(ctx, KMU_E_UNSUPPORTED, "m = %u above KMU_ANCHOR_MAX_NBKMER (%d)", m, KMU_ANCHOR_MAX_NBKMER);
    if ((uint64_t) ndb * n_keys > 0xFFFFFFFFull)
        return fail(ctx, KMU_E_UNSUPPORTED, "%u rows x %u keys: 2^32 index entries or more", ndb, n_keys);
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0 || ndb == 0) return KMU_OK;
    const uint32_t n_entries = ndb * n_keys;

    MatchArgs a{};
    const void *p;
    KMU_TRY(am_to_device(ctx, "am.q", hashes_q, (size_t) nq * m * 8, mem, &p));
    a.q = (const uint64_t *) p;
    if (hashes_db == hashes_q && ndb == nq) a.c.db = a.q; // a self-join is staged once
    else {
        KMU_TRY(am_to_device(ctx, "am.db", hashes_db, (size_t) ndb * m * 8, mem, &p));
        a.c.db = (const uint64_t *) p;
    }
    if (group_q) {
        KMU_TRY(am_to_device(ctx, "am.gq", group_q, (size_t) nq * 4, mem, &p));
        a.gq = (const uint32_t *) p;
        KMU_TRY(am_to_device(ctx, "am.gdb", group_db, (size_t) ndb * 4, mem, &p));
        a.c.gdb = (const uint32_t *) p;
    }
    a.nq = nq;
    a.c.ndb = ndb;
    a.c.m = m;
    a.n_keys = n_keys;
    a.c.min_common = min_common;
    a.n_entries = n_entries;

    // the index
    void *k0, *v0, *k1, *v1, *counts, *offs;
    KMU_TRY(dev_buf(ctx, "am.keys0", (size_t) n_entries * 8, &k0));
    KMU_TRY(dev_buf(ctx, "am.rows0", (size_t) n_entries * 4, &v0));
    KMU_TRY(dev_buf(ctx, "am.keys1", (size_t) n_entries * 8, &k1));
    KMU_TRY(dev_buf(ctx, "am.rows1", (size_t) n_entries * 4, &v1));
    KMU_TRY(dev_buf(ctx, "am.counts", (size_t) nq * 4, &counts));
    KMU_TRY(dev_buf(ctx, "am.offs", ((size_t) nq + 1) * 8, &offs));
    {
        const uint32_t grid = (uint32_t) std::min<uint64_t>(((uint64_t) n_entries + 255) / 256, (uint64_t) ctx->num_cus * 8);
        KernelTimer t(ctx, "k_anchor_entries");
        hipLaunchKernelGGL(k_anchor_entries, dim3(grid), dim3(256), 0, ctx->stream, a.c.db, m, n_keys, n_entries, (uint64_t *) k0,
                           (uint32_t *) v0);
    }
    KMU_HIP(ctx, hipGetLastError());
    KMU_TRY(radix_sort_pairs(ctx, (uint64_t *) k0, (uint32_t *) v0, (uint64_t *) k1, (uint32_t *) v1, n_entries));
    a.skeys = (const uint64_t *) k0;
    a.c.srows = (const uint32_t *) v0;

    // COUNT, offsets, total
    const uint32_t grid = (uint32_t) std::min<uint64_t>(nq, (uint64_t) ctx->num_cus * 32);
    a.counts = (uint32_t *) counts;
    {
        KernelTimer t(ctx, "k_anchor_match_count");
        hipLaunchKernelGGL(k_anchor_match<false>, dim3(grid), dim3(64), 0, ctx->stream, a);
    }
    KMU_HIP(ctx, hipGetLastError());
    KMU_TRY(device_scan_u32(ctx, (const uint32_t *) counts, nq, (uint64_t *) offs));
    uint64_t total = 0;
    KMU_HIP(ctx, hipMemcpyAsync(&total, (const uint64_t *) offs + nq, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    *n_out = total;
    if (!pairs_out || total == 0) return finish_call(ctx, mem);
    if (cap < total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu pairs, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.offs = (const uint64_t *) offs;
    a.c.total = total;
    a.c.pairs = pairs_out;
    a.c.dist = dist_out;
    if (mem == KMU_MEM_HOST) {
        void *d;
        KMU_TRY(dev_buf(ctx, "am.pairs", total * 8, &d));
        a.c.pairs = (uint32_t *) d;
        if (dist_out) {
            KMU_TRY(dev_buf(ctx, "am.dist", total * 12, &d));
            a.c.dist = (uint32_t *) d;
        }
    }
    {
        KernelTimer t(ctx, "k_anchor_match_write");
        hipLaunchKernelGGL(k_anchor_match<true>, dim3(grid), dim3(64), 0, ctx->stream, a);
    }
    KMU_HIP(ctx, hipGetLastError());
    if (mem == KMU_MEM_HOST) {
        KMU_HIP(ctx, hipMemcpyAsync(pairs_out, a.c.pairs, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (dist_out) KMU_HIP(ctx, hipMemcpyAsync(dist_out, a.c.dist, total * 12, hipMemcpyDeviceToHost, ctx->stream));
    }
    return finish_call(ctx, mem);
}

// kmu_anchor_cand.h -- what kmu_anchor_match (kmu_anchor_match.hip) and the anchor index (kmu_anchor_index.hip) share on the device:
// the (key, row) entries of a database and the work on one chunk of 64 candidates of a bucket, so that both walk identically.
#pragma once

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

// entry e = row * n_keys + t is (db[row][t], row), in row order.  The padding of a short row comes along as key u64::MAX.
static __global__ void __launch_bounds__(256) k_anchor_entries(const uint64_t *db, uint32_t m, uint32_t n_keys, uint32_t n_entries,
                                                               uint64_t *keys, uint32_t *rows) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t) (e / n_keys), t = (uint32_t) (e % n_keys);
        keys[e] = db[(uint64_t) row * m + t];
        rows[e] = row;
    }
}

// the database side of a match and where its pairs go
struct CandArgs {
    const uint64_t *db;    // ndb x m
    const uint32_t *gdb;   // group of every database row, or null: no groups
    const uint32_t *srows; // the rows of the entries, sorted by key, ascending inside a key
    uint32_t ndb, m, min_common;
    uint64_t total;         // WRITE: pairs of the whole call
    uint32_t *pairs, *dist; // WRITE: total x 2, total x 3 (dist may be null)
};

// One chunk of a bucket, by one whole wave: lane l has candidate entry e = chunk + l of the bucket that ends at `end` (lanes
// behind the end stand by: every lane reaches the ballot).  `row` is query row r (n1 entries, group g) and row[kk] the key of
// the bucket.  Group test; "is row[kk] the smallest hash under which the pair is seeded" -- a merge of the two rows up to the
// key: a common hash in front of it is a smaller shared key and the pair is reported there, unless `masked` (null: nothing is)
// says that this key of the query is masked: then it seeds nothing and is stepped over --; the walk of k_minhash_distance over
// the whole rows; the min_common filter.  Survivors are compacted in lane order with a ballot and a prefix count behind `at`,
// which moves on by their number (COUNT: only that).
template <bool WRITE>
__device__ __forceinline__ void anchor_candidates(const CandArgs &c, const uint64_t *row, uint32_t n1, uint32_t r, uint32_t g,
                                                  uint32_t kk, const uint8_t *masked, uint32_t e, uint32_t end, uint64_t &at) {
    const uint32_t m = c.m;
    bool pass = e < end;
    uint32_t b = 0, d[3] = {0, 0, 0};
    if (pass) {
        b = c.srows[e];
        pass = b < c.ndb; // (always: an entry names a row of db)
        if (pass && c.gdb) pass = c.gdb[b] != g;
    }
    if (pass) {
        const uint64_t *rb = c.db + (uint64_t) b * m;
        // none in front of row[kk] (rb holds row[kk], so with ascending rows j stays in range; the bound keeps a malformed row
        // from running on)
        uint32_t i = 0, j = 0;
        while (i < kk && j < m) {
            const uint64_t x = row[i], y = rb[j];
            if (x == y) {
                if (!masked || !masked[i]) break;
                i++;
                j++;
            } else if (x < y) i++;
            else j++;
        }
        pass = i == kk;
        if (pass) {
            minhash_walk(row, n1, rb, bottomk_row_len(rb, m), d);
            pass = d[0] >= c.min_common;
        }
    }
    const uint64_t bal = __ballot(pass);
    if (WRITE) {
        const uint64_t o = at + (uint64_t) __popcll(bal & ((1ull << lane_id()) - 1ull));
        if (pass && o < c.total) {
            c.pairs[2 * o] = r;
            c.pairs[2 * o + 1] = b;
            if (c.dist) {
                c.dist[3 * o] = d[0];
                c.dist[3 * o + 1] = d[1];
                c.dist[3 * o + 2] = d[2];
            }
        }
    }
    at += (uint64_t) __popcll(bal);
}

// a host array of a KMU_MEM_HOST call staged in workspace `name`; a device array (or null) as it is
static inline int am_to_device(kmu_ctx *ctx, const char *name, const void *p, size_t bytes, int mem, const void **out) {
    if (mem == KMU_MEM_DEVICE || !p) { *out = p; return KMU_OK; }
    void *d;
    KMU_TRY(dev_buf(ctx, name, bytes ? bytes : 1, &d));
    if (bytes) KMU_HIP(ctx, hipMemcpyAsync(d, p, bytes, hipMemcpyHostToDevice, ctx->stream));
    *out = d;
    return KMU_OK;
}

} // namespace kmu

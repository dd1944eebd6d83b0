// kmu_anchor_db.h -- what kmu_anchor_match.hip and kmu_anchor_index.hip share: the device view of a database side, the arguments
// of the one match kernel, the one build and the one driver.
#pragma once

#include "kmu_ctx.hpp"

namespace kmu {

// A database side as k_anchor_match reads it: in the workspace behind anchor_db_build, or the arrays an anchor index owns.
struct AnchorDb {
    const uint64_t *rows;       // ndb x m
    const uint32_t *groups;     // group of every row, or null: no groups
    const uint32_t *srows;      // the row of every real entry (no padding), by key, ascending inside a key
    const uint64_t *ukeys;      // the distinct keys, ascending
    const uint32_t *ubeg;       // one more than distinct keys: the bucket of ukeys[d] is srows[ubeg[d] .. ubeg[d + 1])
    const uint32_t *n_distinct; // device word: the number of distinct keys (0: every row is empty)
    uint32_t ndb, m, n_keys;
};

struct MatchArgs {
    AnchorDb db;
    const uint64_t *q;  // nq x m
    const uint32_t *gq; // with db.groups: both or neither
    uint32_t nq, min_common, max_occ;
    uint32_t *counts;       // COUNT: pairs of every query row
    const uint64_t *offs;   // WRITE: nq + 1 offsets, offs[nq] = total
    uint64_t total;         // WRITE: pairs of the whole call
    uint32_t *pairs, *dist; // WRITE: total x 2, total x 3 (dist may be null)
};

// kmu_anchor_index.hip.  The directory of db->rows (ndb x m on the device, ndb > 0; db->groups is the caller's) in the context's
// workspace: fills srows, ukeys, ubeg and n_distinct of *db.  Buffers are sized for ndb * n_keys entries, the counts stay on the
// device -- *n_real (may be null) gets the address of the number of real entries --, and nothing here waits for the stream.
int anchor_db_build(kmu_ctx *ctx, AnchorDb *db, const uint32_t **n_real);

// kmu_anchor_match.hip.  COUNT, offsets, the total to the host (the one synchronisation), WRITE, the copies of a host call, and
// finish_call: the end of kmu_anchor_match and of kmu_anchor_index_match.  `a` has its database and query sides filled in.
int anchor_match_run(kmu_ctx *ctx, MatchArgs &a, uint32_t nq, int mem, uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap,
                     uint64_t *n_out);

} // namespace kmu

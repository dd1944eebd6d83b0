// kmu_anchor_index.hip -- the sorted directory of a database side of the anchor join, and the anchor index: that side built once
// and kept on the device (the reference's persistent inverse index smallest hash -> (readnum, slicepos), redis_dump,
// src/anchor.rs:187-197), with the bucket sizes that a repeat mask needs.
//
//  anchor_db_build  for kmu_anchor_match (kmu_anchor_match.hip) and for create, in the workspace, without waiting for the stream:
//           k_anchor_entries  entry e = row * n_keys + t is (db[row][t], row), in row order.  The padding of a short row comes
//                           along as key u64::MAX and sorts to the end.
//           radix_sort_pairs  kmu_sort.h: the entries by key, stable -- ascending rows inside a key, which the output order rests on
//           k_aix_heads     one lane per sorted entry: "this key is not padding and differs from the one before"; the entry behind
//                           which the padding starts leaves the number of real entries
//           device_scan_u32 the flags into directory slots; behind the last, the number of distinct keys
//           k_aix_directory ukeys[d] = the d-th distinct key, ubeg[d] = its first entry, ubeg[n_distinct] = the real entries: the
//                           occupancy of a key (the database rows that have it among their keys) is a subtraction, and the
//                           padding tail is in no bucket.  Both counts stay on the device; the buffers have room for
//                           ndb * n_keys entries.
//  create   anchor_db_build, the two counts to the host, then what only a resident object needs: srows, ukeys, ubeg at their
//           sizes as hipMallocs of the index's own, beside its copy of the rows and the groups (other calls resize the
//           workspace), and k_aix_max_occ: the largest occupancy, wave maximum, one atomic per wave.
//  occupancy  k_aix_occupancy: one lane per distinct key, bins below AIX_LDS_BINS meet in LDS first, one 64-bit atomic per bin
//           and workgroup behind them.
//  match    its own checks and query side, then k_anchor_match through anchor_match_run (kmu_anchor_match.hip) with max_occ.
#include <algorithm>

#include "kmu_anchor_db.h"
#include "kmu_device.h"
#include "kmu_sort.h"

struct kmu_anchor_index {
    kmu_ctx *ctx = nullptr;
    uint32_t ndb = 0, m = 0, n_keys = 0;
    bool has_groups = false;
    uint64_t n_entries = 0, n_distinct = 0; // real entries (no padding), distinct keys
    uint32_t max_occupancy = 0;
    uint64_t device_bytes = 0;
    // the index's own device memory
    uint64_t *rows = nullptr;   // ndb x m
    uint32_t *groups = nullptr; // ndb, or null
    uint32_t *srows = nullptr;  // n_entries: the row of every real entry, by key, ascending inside a key
    uint64_t *ukeys = nullptr;  // n_distinct
    uint32_t *ubeg = nullptr;   // n_distinct + 1
    uint32_t *n_distinct_dev = nullptr; // n_distinct where k_anchor_match reads it
};

namespace kmu {

static constexpr uint32_t AIX_LDS_BINS = 1024;
static constexpr uint64_t PADDING = 0xFFFFFFFFFFFFFFFFull;

// entry e = row * n_keys + t is (db[row][t], row), in row order.  The padding of a short row comes along as key u64::MAX.
__global__ void __launch_bounds__(256) k_anchor_entries(const uint64_t *db, uint32_t m, uint32_t n_keys, uint32_t n_entries, uint64_t *keys,
                                                        uint32_t *rows) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n_entries; e += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t row = (uint32_t) (e / n_keys), t = (uint32_t) (e % n_keys);
        keys[e] = db[(uint64_t) row * m + t];
        rows[e] = row;
    }
}

// flags[e] = 1 where a bucket starts; *n_real = the entries in front of the padding (zeroed by the host: no real entry, no write)
__global__ void __launch_bounds__(256) k_aix_heads(const uint64_t *skeys, uint32_t n, uint32_t *flags, uint32_t *n_real) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t key = skeys[e];
        flags[e] = key != PADDING && (e == 0 || skeys[e - 1] != key);
        if (key != PADDING && (e + 1 == n || skeys[e + 1] == PADDING)) *n_real = (uint32_t) (e + 1);
    }
}

// over all n >= 1 entries (no padding entry has a flag); slot[n] = the distinct keys, which entry 0 leaves in *n_distinct
__global__ void __launch_bounds__(256) k_aix_directory(const uint64_t *skeys, const uint32_t *flags, const uint64_t *slot, uint32_t n,
                                                       const uint32_t *n_real, uint64_t *ukeys, uint32_t *ubeg, uint32_t *n_distinct) {
    const uint64_t nd = slot[n];
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t) gridDim.x * blockDim.x) {
        if (e == 0) {
            ubeg[nd] = *n_real;
            *n_distinct = (uint32_t) nd;
        }
        if (!flags[e]) continue;
        const uint64_t d = slot[e];
        if (d < nd) {
            ukeys[d] = skeys[e];
            ubeg[d] = (uint32_t) e;
        }
    }
}

// whole waves walk the directory: every lane reaches the wave maximum
__global__ void __launch_bounds__(256) k_aix_max_occ(const uint32_t *ubeg, uint32_t n_distinct, uint32_t *out) {
    uint32_t best = 0;
    for (uint64_t d = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; d < n_distinct; d += (uint64_t) gridDim.x * blockDim.x)
        best = max(best, ubeg[d + 1] - ubeg[d]);
    best = wave_max_u32(best);
    if (lane_id() == 0 && best) atomicMax(out, best);
}

// hist[min(occupancy, last_bin)] += 1 for every distinct key; hist has last_bin + 1 bins
__global__ void __launch_bounds__(256) k_aix_occupancy(const uint32_t *ubeg, uint32_t n_distinct, uint32_t last_bin,
                                                       unsigned long long *hist) {
    __shared__ uint32_t bins[AIX_LDS_BINS];
    for (uint32_t i = threadIdx.x; i < AIX_LDS_BINS; i += blockDim.x) bins[i] = 0u;
    __syncthreads();
    for (uint64_t d = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; d < n_distinct; d += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t b = min(ubeg[d + 1] - ubeg[d], last_bin);
        if (b < AIX_LDS_BINS) atomicAdd(&bins[b], 1u);
        else atomicAdd(&hist[b], 1ull); // (keys of a thousand rows and more: rare)
    }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < AIX_LDS_BINS && i <= last_bin; i += blockDim.x)
        if (bins[i]) atomicAdd(&hist[i], (unsigned long long) bins[i]);
}

static int aix_alloc(kmu_anchor_index *ix, void **p, size_t bytes) {
    KMU_HIP(ix->ctx, hipMalloc(p, bytes));
    ix->device_bytes += bytes;
    return KMU_OK;
}

int anchor_db_build(kmu_ctx *ctx, AnchorDb *db, const uint32_t **n_real) {
    const uint32_t n = db->ndb * db->n_keys; // entries, padding included: the host's upper bound of both counts
    uint32_t *ubeg, *flags, *v1, *v0;
    uint64_t *ukeys, *slot, *k1, *k0;
    void *stat;
    KMU_TRY(dev_array(ctx, "am.keys0", (size_t) n, &k0));
    KMU_TRY(dev_array(ctx, "am.rows0", (size_t) n, &v0));
    KMU_TRY(dev_array(ctx, "am.keys1", (size_t) n, &k1));
    KMU_TRY(dev_array(ctx, "am.rows1", (size_t) n, &v1));
    KMU_TRY(dev_array(ctx, "aix.flags", (size_t) n, &flags));
    KMU_TRY(dev_array(ctx, "aix.slot", (size_t) n + 1, &slot));
    KMU_TRY(dev_array(ctx, "aix.ukeys", (size_t) n, &ukeys));
    KMU_TRY(dev_array(ctx, "aix.ubeg", (size_t) n + 1, &ubeg));
    KMU_TRY(dev_buf(ctx, "aix.stat", 8, &stat)); // [0] real entries, [1] distinct keys
    KMU_HIP(ctx, hipMemsetAsync(stat, 0, 8, ctx->stream));
    KMU_TRY(launch(ctx, "k_anchor_entries", k_anchor_entries, dim3(grid_for(ctx, n, 256)), dim3(256), 0, db->rows, db->m, db->n_keys, n, k0, v0));
    KMU_TRY(radix_sort_pairs(ctx, k0, v0, k1, v1, n));
    KMU_TRY(launch(ctx, "k_aix_heads", k_aix_heads, dim3(grid_for(ctx, n, 256)), dim3(256), 0, k0, n, flags, (uint32_t *) stat));
    KMU_TRY(device_scan_u32(ctx, flags, n, slot));
    KMU_TRY(launch(ctx, "k_aix_directory", k_aix_directory, dim3(grid_for(ctx, n, 256)), dim3(256), 0, k0, flags, slot, n, (const uint32_t *) stat,
                   ukeys, ubeg, (uint32_t *) stat + 1));
    db->srows = v0;
    db->ukeys = ukeys;
    db->ubeg = ubeg;
    db->n_distinct = (const uint32_t *) stat + 1;
    if (n_real) *n_real = (const uint32_t *) stat;
    return KMU_OK;
}

// the index as k_anchor_match reads it (before create has built the directory: its rows and groups)
static AnchorDb aix_view(const kmu_anchor_index *ix) {
    return AnchorDb{ix->rows, ix->groups, ix->srows, ix->ukeys, ix->ubeg, ix->n_distinct_dev, ix->ndb, ix->m, ix->n_keys};
}

// everything behind the argument checks of kmu_anchor_index_create; on failure the caller destroys what exists
static int aix_create(kmu_anchor_index *ix, const uint64_t *hashes_db, const uint32_t *group_db, int mem) {
    kmu_ctx *ctx = ix->ctx;
    const uint32_t ndb = ix->ndb, m = ix->m;
    if (ndb == 0) return KMU_OK;
    const hipMemcpyKind up = mem == KMU_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    KMU_TRY(aix_alloc(ix, (void **) &ix->rows, (size_t) ndb * m * 8));
    KMU_HIP(ctx, hipMemcpyAsync(ix->rows, hashes_db, (size_t) ndb * m * 8, up, ctx->stream));
    if (group_db) {
        KMU_TRY(aix_alloc(ix, (void **) &ix->groups, (size_t) ndb * 4));
        KMU_HIP(ctx, hipMemcpyAsync(ix->groups, group_db, (size_t) ndb * 4, up, ctx->stream));
    }
    AnchorDb ws = aix_view(ix); // the index's rows with the directory still in the workspace
    const uint32_t *d_real;
    KMU_TRY(anchor_db_build(ctx, &ws, &d_real));
    const uint64_t n = (uint64_t) ndb * ix->n_keys;
    uint32_t n_real = 0, n_distinct = 0;
    KMU_TRY(read_back(ctx, {{&n_real, d_real}, {&n_distinct, ws.n_distinct}})); // the directory is allocated at its size
    if (n_distinct > n_real || n_real > n) return fail(ctx, KMU_E_HIP, "anchor index: %u keys over %u of %llu entries", n_distinct, n_real, (unsigned long long) n);
    ix->n_entries = n_real;
    ix->n_distinct = n_distinct;
    if (n_distinct == 0) return finish_call(ctx, mem); // every row is empty
    KMU_TRY(aix_alloc(ix, (void **) &ix->srows, (size_t) n_real * 4));
    KMU_TRY(aix_alloc(ix, (void **) &ix->ukeys, (size_t) n_distinct * 8));
    KMU_TRY(aix_alloc(ix, (void **) &ix->ubeg, ((size_t) n_distinct + 1) * 4));
    KMU_TRY(aix_alloc(ix, (void **) &ix->n_distinct_dev, 4));
    KMU_HIP(ctx, hipMemcpyAsync(ix->srows, ws.srows, (size_t) n_real * 4, hipMemcpyDeviceToDevice, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(ix->ukeys, ws.ukeys, (size_t) n_distinct * 8, hipMemcpyDeviceToDevice, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(ix->ubeg, ws.ubeg, ((size_t) n_distinct + 1) * 4, hipMemcpyDeviceToDevice, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(ix->n_distinct_dev, ws.n_distinct, 4, hipMemcpyDeviceToDevice, ctx->stream));
    uint32_t *d_max;
    KMU_TRY(dev_array(ctx, "aix.max_occ", 1, &d_max));
    KMU_HIP(ctx, hipMemsetAsync(d_max, 0, 4, ctx->stream));
    KMU_TRY(launch(ctx, "k_aix_max_occ", k_aix_max_occ, dim3(grid_for(ctx, n_distinct, 256)), dim3(256), 0, (const uint32_t *) ix->ubeg, n_distinct, d_max));
    KMU_TRY(read_back(ctx, {{&ix->max_occupancy, d_max}}));
    // the caller's arrays are free from here on, in both modes
    return finish_synced(ctx);
}

} // namespace kmu

using namespace kmu;

extern "C" {

void kmu_anchor_index_destroy(kmu_anchor_index *ix) {
    if (!ix) return;
    if (ix->ctx) {
        (void) hipSetDevice(ix->ctx->device);
        (void) hipStreamSynchronize(ix->ctx->stream); // a match may still be reading the index
    }
    for (void *p : {(void *) ix->rows, (void *) ix->groups, (void *) ix->srows, (void *) ix->ukeys, (void *) ix->ubeg,
                    (void *) ix->n_distinct_dev})
        if (p) (void) hipFree(p);
    delete ix;
}

int kmu_anchor_index_create(kmu_ctx *ctx, const uint64_t *hashes_db, uint32_t ndb, uint32_t m, uint32_t n_keys, const uint32_t *group_db,
                            int mem, kmu_anchor_index **out) {
    if (!ctx || !hashes_db || !out || m == 0) return fail(ctx, KMU_E_BAD_ARG, "null argument or m == 0");
    *out = nullptr;
    if (n_keys == 0 || n_keys > m) return fail(ctx, KMU_E_BAD_ARG, "n_keys = %u: must be 1 .. m = %u", n_keys, m);
    KMU_TRY(check_mem(ctx, mem));
    if (m > KMU_ANCHOR_MAX_NBKMER) return fail(ctx, KMU_E_UNSUPPORTED, "m = %u above KMU_ANCHOR_MAX_NBKMER (%d)", m, KMU_ANCHOR_MAX_NBKMER);
    if ((uint64_t) ndb * n_keys > 0xFFFFFFFFull)
        return fail(ctx, KMU_E_UNSUPPORTED, "%u rows x %u keys: 2^32 index entries or more", ndb, n_keys);
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    kmu_anchor_index *ix = new kmu_anchor_index();
    ix->ctx = ctx;
    ix->ndb = ndb;
    ix->m = m;
    ix->n_keys = n_keys;
    ix->has_groups = group_db != nullptr;
    const int rc = aix_create(ix, hashes_db, group_db, mem);
    if (rc != KMU_OK) {
        kmu_anchor_index_destroy(ix);
        return rc;
    }
    *out = ix;
    return KMU_OK;
}

int kmu_anchor_index_info(const kmu_anchor_index *ix, kmu_anchor_index_info_t *out) {
    if (!ix || !out) return fail(ix ? ix->ctx : nullptr, KMU_E_BAD_ARG, "null argument");
    *out = kmu_anchor_index_info_t{ix->ndb, ix->m, ix->n_keys, ix->has_groups ? 1u : 0u, ix->n_entries, ix->n_distinct, ix->max_occupancy, 0u,
                                   ix->device_bytes};
    return KMU_OK;
}

int kmu_anchor_index_occupancy(kmu_anchor_index *ix, uint64_t *hist_out, uint32_t n_bins, int mem) {
    if (!ix || !hist_out) return fail(ix ? ix->ctx : nullptr, KMU_E_BAD_ARG, "null argument");
    kmu_ctx *ctx = ix->ctx;
    if (n_bins < 2 || n_bins > 65536) return fail(ctx, KMU_E_BAD_ARG, "n_bins = %u: must be 2 .. 65536", n_bins);
    KMU_TRY(check_mem(ctx, mem));
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t *d_h;
    KMU_TRY(place_output(ctx, "aix.hist", hist_out, (size_t) n_bins, mem, &d_h));
    KMU_HIP(ctx, hipMemsetAsync(d_h, 0, (size_t) n_bins * 8, ctx->stream));
    if (ix->n_distinct) {
        KMU_TRY(launch(ctx, "k_aix_occupancy", k_aix_occupancy, dim3(grid_for(ctx, ix->n_distinct, 256)), dim3(256), 0, (const uint32_t *) ix->ubeg,
                       (uint32_t) ix->n_distinct, n_bins - 1, (unsigned long long *) d_h));
    }
    KMU_TRY(bring_output(ctx, hist_out, d_h, (size_t) n_bins, mem));
    return finish_call(ctx, mem);
}

int kmu_anchor_index_match(kmu_anchor_index *ix, const uint64_t *hashes_q, uint32_t nq, const uint32_t *group_q, uint32_t min_common,
                           uint32_t max_occ, int mem, uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap, uint64_t *n_out) {
    if (!ix || !hashes_q || !n_out) return fail(ix ? ix->ctx : nullptr, KMU_E_BAD_ARG, "null argument");
    kmu_ctx *ctx = ix->ctx;
    if ((group_q != nullptr) != ix->has_groups)
        return fail(ctx, KMU_E_BAD_ARG, "group_q and the index's groups go together: both or neither");
    KMU_TRY(check_mem(ctx, mem));
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0 || ix->n_distinct == 0) return KMU_OK;

    MatchArgs a{};
    KMU_TRY(stage_to_device(ctx, "am.q", hashes_q, (size_t) nq * ix->m, mem, &a.q));
    if (group_q) {
        KMU_TRY(stage_to_device(ctx, "am.gq", group_q, (size_t) nq, mem, &a.gq));
    }
    a.db = aix_view(ix);
    a.min_common = min_common;
    a.max_occ = max_occ;
    return anchor_match_run(ctx, a, nq, mem, pairs_out, dist_out, cap, n_out);
}

} // extern "C"

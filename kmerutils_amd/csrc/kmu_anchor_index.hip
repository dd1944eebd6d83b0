// kmu_anchor_index.hip -- the anchor index: the database side of kmu_anchor_match built once and kept on the device (the
// reference's persistent inverse index smallest hash -> (readnum, slicepos), redis_dump, src/anchor.rs:187-197), with the bucket
// sizes that a repeat mask needs.
//
//  create   k_anchor_entries and radix_sort_pairs as kmu_anchor_match runs them, then a directory of the distinct keys:
//           k_aix_heads     one lane per sorted entry: "this key is not padding and differs from the one before"; the entry behind
//                           which the padding starts leaves the number of real entries
//           device_scan_u32 the flags into directory slots
//           k_aix_directory ukeys[d] = the d-th distinct key, ubeg[d] = its first entry, ubeg[n_distinct] = the real entries: the
//                           occupancy of a key (the database rows that have it among their keys) is a subtraction, and the
//                           padding tail is in no bucket
//           k_aix_max_occ   the largest occupancy: wave maximum, one atomic per wave
//           The sorted keys stay in the workspace and are forgotten; the index owns srows, ukeys, ubeg, the rows and the groups.
//  occupancy  k_aix_occupancy: one lane per distinct key, bins below AIX_LDS_BINS meet in LDS first, one 64-bit atomic per bin
//           and workgroup behind them.
//  match    k_anchor_index_match<COUNT / WRITE>: one wave per query row as in k_anchor_match, but the row's keys are looked up one
//           lane per key -- one binary search in ukeys -- and bucket begin, end and "masked" (max_occ > 0 and occupancy >
//           max_occ) wait in LDS next to the row.  A masked key is skipped without touching its bucket; the candidates of the
//           others go through anchor_candidates (kmu_anchor_cand.h) as k_anchor_match's do, with the flags of the query's own
//           keys: a hash common to both rows and smaller than a shared key is among the keys of both, so a masked common hash in
//           front of the key is one of them and is stepped over.
#include <algorithm>

#include "kmu_anchor_cand.h"
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
};

namespace kmu {

static constexpr uint32_t AIX_LDS_BINS = 1024;
static constexpr uint64_t PADDING = 0xFFFFFFFFFFFFFFFFull;

// flags[e] = 1 where a bucket starts; *n_real = the entries in front of the padding (zeroed by the host: no real entry, no write)
__global__ void __launch_bounds__(256) k_aix_heads(const uint64_t *skeys, uint32_t n, uint32_t *flags, uint32_t *n_real) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t key = skeys[e];
        flags[e] = key != PADDING && (e == 0 || skeys[e - 1] != key);
        if (key != PADDING && (e + 1 == n || skeys[e + 1] == PADDING)) *n_real = (uint32_t) (e + 1);
    }
}

__global__ void __launch_bounds__(256) k_aix_directory(const uint64_t *skeys, const uint32_t *flags, const uint64_t *slot,
                                                       uint32_t n_real, uint32_t n_distinct, uint64_t *ukeys, uint32_t *ubeg) {
    for (uint64_t e = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; e < n_real; e += (uint64_t) gridDim.x * blockDim.x) {
        if (e == 0) ubeg[n_distinct] = n_real;
        if (!flags[e]) continue;
        const uint64_t d = slot[e];
        if (d < n_distinct) {
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

struct IndexMatchArgs {
    const uint64_t *q; // nq x m
    uint32_t nq, n_keys, max_occ;
    const uint32_t *gq;    // with c.gdb: both or neither
    const uint64_t *ukeys; // n_distinct distinct keys, ascending
    const uint32_t *ubeg;  // n_distinct + 1: the bucket of ukeys[d] is c.srows[ubeg[d] .. ubeg[d + 1])
    uint32_t n_distinct;
    uint32_t *counts;     // COUNT: pairs of every query row
    const uint64_t *offs; // WRITE: nq + 1 offsets, offs[nq] = total
    CandArgs c;
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_anchor_index_match(IndexMatchArgs a) {
    __shared__ uint64_t row[KMU_ANCHOR_MAX_NBKMER];
    __shared__ uint32_t kbeg[KMU_ANCHOR_MAX_NBKMER], kend[KMU_ANCHOR_MAX_NBKMER]; // the bucket of every key of the row
    __shared__ uint8_t kmask[KMU_ANCHOR_MAX_NBKMER];                              // 1: the key is masked
    const uint32_t lane = (uint32_t) lane_id(), m = a.c.m;
    for (uint32_t r = blockIdx.x; r < a.nq; r += gridDim.x) {
        uint32_t n1 = 0;
        for (uint32_t t0 = 0; t0 < m; t0 += 64) { // uniform trip count
            const uint32_t t = t0 + lane;
            const uint64_t h = t < m ? a.q[(uint64_t) r * m + t] : PADDING;
            if (t < m) row[t] = h;
            n1 += (uint32_t) __popcll(__ballot(h != PADDING));
        }
        __syncthreads();
        const uint32_t nk = min(a.n_keys, n1);
        for (uint32_t t = lane; t < nk; t += 64) { // one lane per key
            const uint64_t key = row[t];
            uint32_t lo = 0, hi = a.n_distinct;
            while (lo < hi) { // first distinct key >= key
                const uint32_t mid = lo + (hi - lo) / 2;
                if (a.ukeys[mid] < key) lo = mid + 1;
                else hi = mid;
            }
            uint32_t beg = 0, end = 0;
            if (lo < a.n_distinct && a.ukeys[lo] == key) {
                beg = a.ubeg[lo];
                end = a.ubeg[lo + 1];
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
                anchor_candidates<WRITE>(a.c, row, n1, r, g, kk, kmask, c + lane, end, at);
        }
        if (!WRITE && lane == 0) a.counts[r] = (uint32_t) at;
        __syncthreads(); // the next row overwrites the LDS copies
    }
}

static uint32_t aix_grid(kmu_ctx *ctx, uint64_t n) {
    return (uint32_t) std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t) ctx->num_cus * 8));
}

static int aix_alloc(kmu_anchor_index *ix, void **p, size_t bytes) {
    KMU_HIP(ix->ctx, hipMalloc(p, bytes));
    ix->device_bytes += bytes;
    return KMU_OK;
}

// everything behind the argument checks of kmu_anchor_index_create; on failure the caller destroys what exists
static int aix_build(kmu_anchor_index *ix, const uint64_t *hashes_db, const uint32_t *group_db, int mem) {
    kmu_ctx *ctx = ix->ctx;
    const uint32_t ndb = ix->ndb, m = ix->m, n_keys = ix->n_keys;
    if (ndb == 0) return KMU_OK;
    const hipMemcpyKind up = mem == KMU_MEM_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    KMU_TRY(aix_alloc(ix, (void **) &ix->rows, (size_t) ndb * m * 8));
    KMU_HIP(ctx, hipMemcpyAsync(ix->rows, hashes_db, (size_t) ndb * m * 8, up, ctx->stream));
    if (group_db) {
        KMU_TRY(aix_alloc(ix, (void **) &ix->groups, (size_t) ndb * 4));
        KMU_HIP(ctx, hipMemcpyAsync(ix->groups, group_db, (size_t) ndb * 4, up, ctx->stream));
    }
    const uint32_t n = ndb * n_keys; // entries, padding included
    void *k0, *v0, *k1, *v1, *flags, *slot, *stat;
    KMU_TRY(dev_buf(ctx, "am.keys0", (size_t) n * 8, &k0));
    KMU_TRY(dev_buf(ctx, "am.rows0", (size_t) n * 4, &v0));
    KMU_TRY(dev_buf(ctx, "am.keys1", (size_t) n * 8, &k1));
    KMU_TRY(dev_buf(ctx, "am.rows1", (size_t) n * 4, &v1));
    KMU_TRY(dev_buf(ctx, "aix.flags", (size_t) n * 4, &flags));
    KMU_TRY(dev_buf(ctx, "aix.slot", ((size_t) n + 1) * 8, &slot));
    KMU_TRY(dev_buf(ctx, "aix.stat", 8, &stat)); // [0] real entries, [1] largest occupancy
    KMU_HIP(ctx, hipMemsetAsync(stat, 0, 8, ctx->stream));
    {
        KernelTimer t(ctx, "k_anchor_entries");
        hipLaunchKernelGGL(k_anchor_entries, dim3(aix_grid(ctx, n)), dim3(256), 0, ctx->stream, (const uint64_t *) ix->rows, m, n_keys, n,
                           (uint64_t *) k0, (uint32_t *) v0);
    }
    KMU_HIP(ctx, hipGetLastError());
    KMU_TRY(radix_sort_pairs(ctx, (uint64_t *) k0, (uint32_t *) v0, (uint64_t *) k1, (uint32_t *) v1, n));
    {
        KernelTimer t(ctx, "k_aix_heads");
        hipLaunchKernelGGL(k_aix_heads, dim3(aix_grid(ctx, n)), dim3(256), 0, ctx->stream, (const uint64_t *) k0, n, (uint32_t *) flags,
                           (uint32_t *) stat);
    }
    KMU_HIP(ctx, hipGetLastError());
    KMU_TRY(device_scan_u32(ctx, (const uint32_t *) flags, n, (uint64_t *) slot));
    uint64_t n_distinct = 0;
    uint32_t h_stat[2] = {0, 0};
    KMU_HIP(ctx, hipMemcpyAsync(&n_distinct, (const uint64_t *) slot + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(h_stat, stat, 4, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream)); // the directory is allocated at its size
    const uint32_t n_real = h_stat[0];
    if (n_distinct > n_real || n_real > n) return fail(ctx, KMU_E_HIP, "anchor index: %llu keys over %u of %u entries", (unsigned long long) n_distinct, n_real, n);
    ix->n_entries = n_real;
    ix->n_distinct = n_distinct;
    if (n_distinct == 0) return finish_call(ctx, mem); // every row is empty
    KMU_TRY(aix_alloc(ix, (void **) &ix->srows, (size_t) n_real * 4));
    KMU_TRY(aix_alloc(ix, (void **) &ix->ukeys, (size_t) n_distinct * 8));
    KMU_TRY(aix_alloc(ix, (void **) &ix->ubeg, ((size_t) n_distinct + 1) * 4));
    KMU_HIP(ctx, hipMemcpyAsync(ix->srows, v0, (size_t) n_real * 4, hipMemcpyDeviceToDevice, ctx->stream));
    {
        KernelTimer t(ctx, "k_aix_directory");
        hipLaunchKernelGGL(k_aix_directory, dim3(aix_grid(ctx, n_real)), dim3(256), 0, ctx->stream, (const uint64_t *) k0,
                           (const uint32_t *) flags, (const uint64_t *) slot, n_real, (uint32_t) n_distinct, ix->ukeys, ix->ubeg);
    }
    KMU_HIP(ctx, hipGetLastError());
    {
        KernelTimer t(ctx, "k_aix_max_occ");
        hipLaunchKernelGGL(k_aix_max_occ, dim3(aix_grid(ctx, n_distinct)), dim3(256), 0, ctx->stream, (const uint32_t *) ix->ubeg,
                           (uint32_t) n_distinct, (uint32_t *) stat + 1);
    }
    KMU_HIP(ctx, hipGetLastError());
    KMU_HIP(ctx, hipMemcpyAsync(&ix->max_occupancy, (const uint32_t *) stat + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    // the caller's arrays are free from here on, in both modes
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->profiling) profile_collect(ctx);
    return KMU_OK;
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
    for (void *p : {(void *) ix->rows, (void *) ix->groups, (void *) ix->srows, (void *) ix->ukeys, (void *) ix->ubeg})
        if (p) (void) hipFree(p);
    delete ix;
}

int kmu_anchor_index_create(kmu_ctx *ctx, const uint64_t *hashes_db, uint32_t ndb, uint32_t m, uint32_t n_keys, const uint32_t *group_db,
                            int mem, kmu_anchor_index **out) {
    if (!ctx || !hashes_db || !out || m == 0) return fail(ctx, KMU_E_BAD_ARG, "null argument or m == 0");
    *out = nullptr;
    if (n_keys == 0 || n_keys > m) return fail(ctx, KMU_E_BAD_ARG, "n_keys = %u: must be 1 .. m = %u", n_keys, m);
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
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
    const int rc = aix_build(ix, hashes_db, group_db, mem);
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
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t *d_h = hist_out;
    if (mem == KMU_MEM_HOST) {
        void *q;
        KMU_TRY(dev_buf(ctx, "aix.hist", (size_t) n_bins * 8, &q));
        d_h = (uint64_t *) q;
    }
    KMU_HIP(ctx, hipMemsetAsync(d_h, 0, (size_t) n_bins * 8, ctx->stream));
    if (ix->n_distinct) {
        KernelTimer t(ctx, "k_aix_occupancy");
        hipLaunchKernelGGL(k_aix_occupancy, dim3(aix_grid(ctx, ix->n_distinct)), dim3(256), 0, ctx->stream, (const uint32_t *) ix->ubeg,
                           (uint32_t) ix->n_distinct, n_bins - 1, (unsigned long long *) d_h);
        KMU_HIP(ctx, hipGetLastError());
    }
    if (mem == KMU_MEM_HOST) KMU_HIP(ctx, hipMemcpyAsync(hist_out, d_h, (size_t) n_bins * 8, hipMemcpyDeviceToHost, ctx->stream));
    return finish_call(ctx, mem);
}

int kmu_anchor_index_match(kmu_anchor_index *ix, const uint64_t *hashes_q, uint32_t nq, const uint32_t *group_q, uint32_t min_common,
                           uint32_t max_occ, int mem, uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap, uint64_t *n_out) {
    if (!ix || !hashes_q || !n_out) return fail(ix ? ix->ctx : nullptr, KMU_E_BAD_ARG, "null argument");
    kmu_ctx *ctx = ix->ctx;
    if ((group_q != nullptr) != ix->has_groups)
        return fail(ctx, KMU_E_BAD_ARG, "group_q and the index's groups go together: both or neither");
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0 || ix->n_distinct == 0) return KMU_OK;
    const uint32_t m = ix->m;

    IndexMatchArgs a{};
    const void *p;
    KMU_TRY(am_to_device(ctx, "am.q", hashes_q, (size_t) nq * m * 8, mem, &p));
    a.q = (const uint64_t *) p;
    if (group_q) {
        KMU_TRY(am_to_device(ctx, "am.gq", group_q, (size_t) nq * 4, mem, &p));
        a.gq = (const uint32_t *) p;
    }
    a.nq = nq;
    a.n_keys = ix->n_keys;
    a.max_occ = max_occ;
    a.ukeys = ix->ukeys;
    a.ubeg = ix->ubeg;
    a.n_distinct = (uint32_t) ix->n_distinct;
    a.c.db = ix->rows;
    a.c.gdb = ix->groups;
    a.c.srows = ix->srows;
    a.c.ndb = ix->ndb;
    a.c.m = m;
    a.c.min_common = min_common;

    // COUNT, offsets, total
    void *counts, *offs;
    KMU_TRY(dev_buf(ctx, "am.counts", (size_t) nq * 4, &counts));
    KMU_TRY(dev_buf(ctx, "am.offs", ((size_t) nq + 1) * 8, &offs));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(nq, (uint64_t) ctx->num_cus * 32);
    a.counts = (uint32_t *) counts;
    {
        KernelTimer t(ctx, "k_anchor_index_match_count");
        hipLaunchKernelGGL(k_anchor_index_match<false>, dim3(grid), dim3(64), 0, ctx->stream, a);
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
        KernelTimer t(ctx, "k_anchor_index_match_write");
        hipLaunchKernelGGL(k_anchor_index_match<true>, dim3(grid), dim3(64), 0, ctx->stream, a);
    }
    KMU_HIP(ctx, hipGetLastError());
    if (mem == KMU_MEM_HOST) {
        KMU_HIP(ctx, hipMemcpyAsync(pairs_out, a.c.pairs, total * 8, hipMemcpyDeviceToHost, ctx->stream));
        if (dist_out) KMU_HIP(ctx, hipMemcpyAsync(dist_out, a.c.dist, total * 12, hipMemcpyDeviceToHost, ctx->stream));
    }
    return finish_call(ctx, mem);
}

} // extern "C"

// kmu_knn.hip -- exact k-nearest-neighbour search over signature rows (kmu_sig_knn).
//
// What the reference's `datasketcher ... ann` asks of an HNSW index under DistHamming / DistBlockSketched
// (src/bin/datasketcher.rs:98-109, 137-192, 261-309; src/sketching/seqblocksketch.rs:419-440), answered exactly: every
// query row is compared with every database row (slot equality, as k_sig_equal_matrix does) and the selection of the k
// best rows is fused behind the compare, so no count is ever written to memory.
//
// One total order makes the result a pure function of the inputs:  key = eq << 32 | (0xFFFFFFFF - j), larger is better
// (eq descending, then row index ascending).  A valid key is never 0 (j <= 0xFFFFFFFE), so 0 stands for "no entry".
//
//  k_sig_knn        grid (query tiles, database segments).  A workgroup keeps a 64-row query tile and walks the 64-row
//                   tiles of its segment past it; each thread owns a 4 x 4 block of counters as in k_sig_equal_matrix.
//                   The best-k keys of every query row live in LDS, sorted descending; list[k - 1] is the entry
//                   threshold.  The 16 threads that hold counters of one query row sit in ONE wave (row = ty + 16 r,
//                   wave = ty >> 2), so a row's list has a single owner wave and insertion needs no workgroup barrier.
//  k_sig_knn_merge  one wave per query row: merges the sorted partial lists of the segments (lane l holds entry l) and
//                   turns keys into (idx, eq).
#include <algorithm>
#include <cstdlib>

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

static constexpr int KT = 64;            // rows of a query tile and of a database tile
static constexpr int KCHUNK_BYTES = 128; // slots go through LDS in chunks of 128 bytes per row (32 u32 / 16 u64 words)

// Number of differing slots among the 16 bytes of a and of b (four u32 slots or two u64 slots, one ds_read_b128 each).
// Counting the slots that DIFFER lets the compiler pair them: per two slots two v_cmp_ne, one v_cndmask and one
// v_addc_co that adds the select and the second compare's carry -- 2 instructions per slot (2.5 issue slots, the carry
// add being half rate), where `acc += a == b` is a compare, a select and an add per slot.
template <typename W> __device__ __forceinline__ uint32_t differing_slots(uint4 a, uint4 b) {
    if constexpr (sizeof(W) == 4)
        return min(a.x ^ b.x, 1u) + min(a.y ^ b.y, 1u) + min(a.z ^ b.z, 1u) + min(a.w ^ b.w, 1u);
    else
        return min((a.x ^ b.x) | (a.y ^ b.y), 1u) + min((a.z ^ b.z) | (a.w ^ b.w), 1u);
}

// best-k keys of the 64 query rows of a workgroup, [KT][K], descending per row.  Volatile: a row's list is read and
// written by the lanes of its owner wave between workgroup barriers, in program order.
extern __shared__ volatile uint64_t knn_keys[];

// insert `key` into the descending list of K keys that starts at knn_keys[base] (one wave, all 64 lanes active, lane l
// owns entry l: every lane reads before any lane writes).  A key below every entry leaves the list unchanged.
__device__ __forceinline__ void knn_insert(uint32_t base, uint32_t K, uint32_t lane, uint64_t key) {
    if (lane < K) {
        const uint64_t cur = knn_keys[base + lane];
        const uint64_t prev = lane ? knn_keys[base + lane - 1] : ~0ull;
        knn_keys[base + lane] = cur > key ? cur : (prev > key ? key : prev);
    }
}

template <typename W>
__global__ void __launch_bounds__(256) k_sig_knn(const W *__restrict__ q, uint32_t nq, const W *__restrict__ db, uint32_t ndb,
                                                 uint32_t m, uint32_t K, uint32_t seg_rows, const uint32_t *__restrict__ gq,
                                                 const uint32_t *__restrict__ gdb, uint64_t *__restrict__ part) {
    constexpr int MC = KCHUNK_BYTES / (int) sizeof(W); // slots per chunk
    constexpr int TV = 16 / (int) sizeof(W);           // slots per 16-byte LDS read
    constexpr int NLD = KT * MC / 256;                 // words of each side a thread stages per chunk (8 / 4)
    constexpr int RSTEP = 256 / MC;                    // rows between two words of one thread
    // row stride 36 dwords: rows stay 16-byte aligned, and the 16 rows that one lane group of a ds_read_b128 touches
    // start at banks 36 r mod 64 = 0, 36, 8, 44, ...: sixteen disjoint runs of four banks
    __shared__ __attribute__((aligned(16))) W la[KT][MC + TV], lb[KT][MC + TV];

    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const uint32_t tx = tid & 15u, ty = tid >> 4;
    const uint32_t i0 = blockIdx.x * KT;
    const uint32_t jbeg = blockIdx.y * seg_rows; // < ndb
    const uint32_t jend = (uint32_t) min((uint64_t) ndb, (uint64_t) jbeg + seg_rows);
    const uint32_t lrow = tid / MC, lt = tid % MC;    // staging position of this thread
    const uint32_t m_staged = (m + MC - 1) / MC * MC; // slots compared per pair; the padding slots always differ

    for (uint32_t e = tid; e < KT * K; e += 256) knn_keys[e] = 0;
    uint32_t my_group[4];
#pragma unroll
    for (int r = 0; r < 4; r++) {
        const uint32_t i = i0 + ty + 16 * r;
        my_group[r] = (gq && i < nq) ? gq[i] : 0;
    }

    W ra[NLD], rb[NLD];
    // slots past m and rows past the end are filled with values that differ between the two sides
    auto fetch = [&](uint32_t j0, uint32_t t0) {
#pragma unroll
        for (int u = 0; u < NLD; u++) {
            const uint32_t row = lrow + RSTEP * u, t = t0 + lt;
            ra[u] = (i0 + row < nq && t < m) ? q[(uint64_t) (i0 + row) * m + t] : (W) 0;
            rb[u] = (j0 + row < jend && t < m) ? db[(uint64_t) (j0 + row) * m + t] : (W) 1;
        }
    };

    uint32_t diff[4][4];
    fetch(jbeg, 0);
    for (uint32_t j0 = jbeg; j0 < jend; j0 += KT) {
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
            for (int c = 0; c < 4; c++) diff[r][c] = 0;
        for (uint32_t t0 = 0; t0 < m; t0 += MC) {
            __syncthreads(); // the previous chunk has been consumed (and, first time round, the lists are zeroed)
#pragma unroll
            for (int u = 0; u < NLD; u++) {
                la[lrow + RSTEP * u][lt] = ra[u];
                lb[lrow + RSTEP * u][lt] = rb[u];
            }
            __syncthreads();
            // request the next chunk (of this tile, or the first of the next tile) while this one is compared
            if (t0 + MC < m) fetch(j0, t0 + MC);
            else if (j0 + KT < jend) fetch(j0 + KT, 0);
#pragma unroll 2
            for (int t = 0; t < MC; t += TV) {
                uint4 va[4], vb[4];
#pragma unroll
                for (int r = 0; r < 4; r++) va[r] = *reinterpret_cast<const uint4 *>(&la[ty + 16 * r][t]);
#pragma unroll
                for (int c = 0; c < 4; c++) vb[c] = *reinterpret_cast<const uint4 *>(&lb[tx + 16 * c][t]);
#pragma unroll
                for (int r = 0; r < 4; r++)
#pragma unroll
                    for (int c = 0; c < 4; c++) diff[r][c] += differing_slots<W>(va[r], vb[c]);
            }
        }
        // selection: almost every candidate fails the one compare against its row's threshold
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const uint32_t row = ty + 16 * r, i = i0 + row;
            uint64_t thr = knn_keys[row * K + K - 1];
#pragma unroll
            for (int c = 0; c < 4; c++) {
                const uint32_t j = j0 + tx + 16 * c;
                const uint64_t key = ((uint64_t) (m_staged - diff[r][c]) << 32) | (uint64_t) (0xFFFFFFFFu - j);
                // rows past the end are rejected explicitly: eq = 0 is a legal candidate
                bool pass = key > thr && j < jend && i < nq;
                if (pass && gq) pass = gdb[j] != my_group[r];
                uint64_t todo = __ballot(pass);
                if (todo) {
                    while (todo) {
                        const int src = __ffsll((long long) todo) - 1;
                        todo &= todo - 1;
                        const uint32_t srow = (uint32_t) __shfl((int) row, src);
                        const uint32_t hi = (uint32_t) __shfl((int) (uint32_t) (key >> 32), src);
                        const uint32_t lo = (uint32_t) __shfl((int) (uint32_t) key, src);
                        knn_insert(srow * K, K, lane, ((uint64_t) hi << 32) | lo);
                    }
                    thr = knn_keys[row * K + K - 1];
                }
            }
        }
    }
    __syncthreads();
    // partial list of (segment, query row): part[(segment * nq + i) * K + l]
    for (uint32_t e = tid; e < KT * K; e += 256) {
        const uint32_t i = i0 + e / K;
        if (i < nq) part[((uint64_t) blockIdx.y * nq + i) * K + e % K] = knn_keys[e];
    }
}

// one wave per query row; lane l holds entry l of the merged list
__global__ void __launch_bounds__(256) k_sig_knn_merge(const uint64_t *__restrict__ part, uint32_t nq, uint32_t nseg, uint32_t K,
                                                       uint32_t *__restrict__ idx_out, uint16_t *__restrict__ eq_out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t i = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= nq) return; // whole waves leave
    uint64_t best = 0;
    for (uint32_t s = 0; s < nseg; s++) {
        const uint64_t v = lane < K ? part[((uint64_t) s * nq + i) * K + lane] : 0;
        for (uint32_t x = 0; x < K; x++) {
            const uint64_t key = (uint64_t) __shfl((long long) v, (int) x);
            const uint64_t last = (uint64_t) __shfl((long long) best, (int) (K - 1));
            if (key <= last) break; // the segment's list is descending, "no entry" is 0: nothing further can enter
            uint64_t prev = (uint64_t) __shfl_up((long long) best, 1);
            if (lane == 0) prev = ~0ull;
            best = best > key ? best : (prev > key ? key : prev);
        }
    }
    if (lane < K) {
        idx_out[(uint64_t) i * K + lane] = 0xFFFFFFFFu - (uint32_t) best; // best == 0: KMU_KNN_NONE, eq 0
        eq_out[(uint64_t) i * K + lane] = (uint16_t) (best >> 32);
    }
}

static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long long v = atoll(e);
    return v > 0 ? (uint64_t) v : dflt;
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_sig_knn(kmu_ctx *ctx, const void *sig_q, uint32_t nq, const void *sig_db, uint32_t ndb, uint32_t m,
                           int sig_type, uint32_t k, const uint32_t *group_q, const uint32_t *group_db, int mem,
                           uint32_t *idx_out, uint16_t *eq_out) {
    if (!ctx || m == 0 || k == 0 || !sig_q || !sig_db || !idx_out || !eq_out)
        return fail(ctx, KMU_E_BAD_ARG, "null argument, m == 0 or k == 0");
    if (sig_type < KMU_SIG_U32 || sig_type > KMU_SIG_F64) return fail(ctx, KMU_E_BAD_ARG, "bad sig_type %d", sig_type);
    if ((group_q == nullptr) != (group_db == nullptr))
        return fail(ctx, KMU_E_BAD_ARG, "group_q and group_db go together: both null or both given");
    if (m > 65535u) return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %u does not fit the 16-bit counts of the lists", m);
    if (k > KMU_KNN_MAX_K) return fail(ctx, KMU_E_UNSUPPORTED, "k = %u is above KMU_KNN_MAX_K = %d", k, KMU_KNN_MAX_K);
    if (ndb == 0xFFFFFFFFu) return fail(ctx, KMU_E_UNSUPPORTED, "row index 0xFFFFFFFF is KMU_KNN_NONE: at most 2^32 - 2 database rows");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (nq == 0) return KMU_OK;
    const int wb = (sig_type == KMU_SIG_U32 || sig_type == KMU_SIG_F32) ? 4 : 8;
    uint32_t *didx;
    uint16_t *deq;
    const size_t n_out = (size_t) nq * k;
    KMU_TRY(place_output(ctx, "knn.idx", idx_out, n_out, mem, &didx));
    KMU_TRY(place_output(ctx, "knn.eq", eq_out, n_out, mem, &deq));
    if (ndb == 0) { // every list is "none"
        KMU_HIP(ctx, hipMemsetAsync(didx, 0xFF, n_out * 4, ctx->stream));
        KMU_HIP(ctx, hipMemsetAsync(deq, 0, n_out * 2, ctx->stream));
    } else {
        const void *dq, *ddb;
        const uint32_t *dgq = nullptr, *dgdb = nullptr;
        KMU_TRY(stage_to_device(ctx, "knn.q", sig_q, (size_t) nq * m * wb, mem, &dq));
        if (sig_db == sig_q && ndb == nq) ddb = dq; // a self-join is staged once
        else KMU_TRY(stage_to_device(ctx, "knn.db", sig_db, (size_t) ndb * m * wb, mem, &ddb));
        if (group_q) {
            KMU_TRY(stage_to_device(ctx, "knn.gq", group_q, (size_t) nq, mem, &dgq));
            KMU_TRY(stage_to_device(ctx, "knn.gdb", group_db, (size_t) ndb, mem, &dgdb));
        }
        // database segments: enough workgroups for every CU a few times over, no more (each segment costs a partial list
        // per query row).  KMU_KNN_SEG_ROWS fixes the segment height (tests: several segments on a small database).
        const uint32_t qtiles_all = (nq + KT - 1) / KT, dbtiles = (ndb + KT - 1) / KT;
        uint64_t seg_rows = env_u64("KMU_KNN_SEG_ROWS", 0);
        if (!seg_rows) {
            const uint64_t want = std::min<uint64_t>(dbtiles, ((uint64_t) ctx->num_cus * 4 + qtiles_all - 1) / qtiles_all);
            seg_rows = (dbtiles + want - 1) / want * KT;
        }
        seg_rows = (seg_rows + KT - 1) / KT * KT;
        seg_rows = std::max<uint64_t>(seg_rows, (((uint64_t) ndb + 65534u) / 65535u + KT - 1) / KT * KT); // gridDim.y <= 65535
        seg_rows = std::min<uint64_t>(seg_rows, (uint64_t) dbtiles * KT);
        const uint32_t nseg = (uint32_t) ((ndb + seg_rows - 1) / seg_rows);
        // query slabs: the partial lists of one slab (rows x nseg x k keys) stay within the workspace bound
        // (KMU_KNN_WS_MB, tests: several slabs on a small query set)
        const uint64_t ws_bytes = env_u64("KMU_KNN_WS_MB", 256) << 20;
        uint64_t slab = ws_bytes / ((uint64_t) nseg * k * 8) / KT * KT;
        slab = std::min<uint64_t>(std::max<uint64_t>(slab, KT), (uint64_t) qtiles_all * KT);
        uint64_t *dpart;
        KMU_TRY(dev_array(ctx, "knn.part", std::min<uint64_t>(slab, nq) * nseg * k, &dpart));
        for (uint64_t s0 = 0; s0 < nq; s0 += slab) {
            const uint32_t rows = (uint32_t) std::min<uint64_t>(slab, nq - s0);
            const dim3 grid((rows + KT - 1) / KT, nseg);
            const size_t dyn = (size_t) KT * k * 8;
            const uint32_t *gqs = dgq ? dgq + s0 : nullptr;
            if (wb == 4)
                KMU_TRY(launch(ctx, "k_sig_knn", k_sig_knn<uint32_t>, grid, dim3(256), dyn, (const uint32_t *) dq + s0 * m, rows, ddb, ndb, m, k,
                               (uint32_t) seg_rows, gqs, dgdb, dpart));
            else
                KMU_TRY(launch(ctx, "k_sig_knn", k_sig_knn<uint64_t>, grid, dim3(256), dyn, (const uint64_t *) dq + s0 * m, rows, ddb, ndb, m, k,
                               (uint32_t) seg_rows, gqs, dgdb, dpart));
            KMU_TRY(launch(ctx, "k_sig_knn_merge", k_sig_knn_merge, dim3((rows + 3) / 4), dim3(256), 0, dpart, rows, nseg, k, didx + s0 * k,
                           deq + s0 * k));
        }
    }
    KMU_TRY(bring_output(ctx, idx_out, didx, n_out, mem));
    KMU_TRY(bring_output(ctx, eq_out, deq, n_out, mem));
    return finish_call(ctx, mem);
}

// kmu_count_read.hip -- reading the count table back: the count spectrum of the table (kmu_count_histogram) and
// the abundance of the k-mers of reads in it, per position and summarised per read (kmu_count_read_profile).  Neither has a
// counterpart upstream (the reference's filters cannot be enumerated without a dump).
//
// Three kernels and two small ones:
//  * k_count_hist: one streaming pass over the slots (the shape of k_count_stats).  Counts 1 and 2 -- most of a real spectrum -- are
//    counted in registers, the other counts below 256 in per-wave LDS sub-histograms, the rare ones above in global memory; one
//    64-bit global add per non-zero bin and block at the end.
//  * k_count_profile: the flat-stream wave step (kmu_flat.h), one look-up per k-mer, the clamped count stored as uint16.
//  * k_profile_stats: per read, from the uint16 counts: wave reductions, and the exact median by counting (a 256-bin LDS histogram
//    of the high byte, then of the low byte inside the selected bin; 8-bit counters: one round).  Two shapes, chosen per read:
//    one WAVE per read up to PROFILE_SHORT_MAX k-mers, one BLOCK per read above.
//  * k_profile_big_accum / k_profile_big_finish: a read longer than the bounded workspace (stats without counts_out), over
//    sub-ranges: many blocks add into one global histogram of every count value, one block picks the median out of it.
#include <algorithm>
#include <vector>

#include "kmu_count_plan.hpp"
#include "kmu_count_table.h"
#include "kmu_flat.h"

namespace kmu {

// ------------------------------------------------------------------------------------------------
// the count spectrum
// ------------------------------------------------------------------------------------------------
// hist[v] += slots whose reported count (clamped to maxc, then folded into last_bin) is v; hist has last_bin + 1 bins
__global__ void __launch_bounds__(256) k_count_hist(CountTable t, uint64_t nslots, uint32_t maxc, uint32_t last_bin,
                                                    unsigned long long *hist) {
    __shared__ uint32_t sub[4][256]; // one sub-histogram per wave: no LDS atomic of one wave waits for another wave's
    const int wave = threadIdx.x >> 6;
    for (uint32_t i = threadIdx.x; i < 1024u; i += 256u) (&sub[0][0])[i] = 0u;
    __syncthreads();
    uint32_t n1 = 0, n2 = 0; // the two hot bins never reach LDS: a lane sees < 2^32 slots (grid_for)
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t key;
        uint32_t c; // 0: an entry that left for its owner (distributed counters): absent for every reader
        if (slot_read<false>(t, i, key, c) && c != 0u) {
            uint32_t v = c > maxc ? maxc : c;
            v = v > last_bin ? last_bin : v;
            if (v == 1u) n1++;
            else if (v == 2u) n2++;
            else if (v < 256u) atomicAdd(&sub[wave][v], 1u);
            else atomicAdd(&hist[v], 1ull); // (16-bit counters only, and rare)
        }
    }
    n1 = wave_sum_u32(n1);
    n2 = wave_sum_u32(n2);
    if (lane_id() == 0) {
        sub[wave][1] = n1; // (bins 1 and 2 of the sub-histograms are written here only)
        if (last_bin >= 2u) sub[wave][2] = n2;
    }
    __syncthreads();
    const uint32_t b = threadIdx.x;
    const uint64_t s = (uint64_t) sub[0][b] + sub[1][b] + sub[2][b] + sub[3][b];
    if (s && b <= last_bin) atomicAdd(&hist[b], (unsigned long long) s);
}

// ------------------------------------------------------------------------------------------------
// per-position counts of the k-mers of reads
// ------------------------------------------------------------------------------------------------
// Wave steps [st0, st1) of the flat stream; the k-mer starting at base g of the stream, lo <= g < hi, inside one read:
// counts[g - cbase] = min(count of its canonical value, maxc).  Positions that start no k-mer are not written.  cbase is a
// multiple of 1024, `vec`: counts is 16-byte aligned (a lane's 16 counts then go out as two 16-byte stores where all are valid).
// `empty`: the table holds nothing (and may not exist): every k-mer is absent, no slot is read.
__global__ void __launch_bounds__(256) k_count_profile(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k,
                                                       CountTable t, int empty, uint32_t maxc, uint64_t st0, uint64_t st1,
                                                       uint64_t lo, uint64_t hi, uint16_t *counts, uint64_t cbase, int vec,
                                                       uint32_t *err) {
    const uint64_t total = offsets[n_seq], start = offsets[0];
    if (lo < start) lo = start;
    if (hi > total) hi = total;
    const uint64_t wave_global = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves_global = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    uint32_t r_hint = 0xFFFFFFFFu, anybad = 0;
    for (uint64_t st = st0 + wave_global; st < st1; st += nwaves_global) {
        const uint64_t g0 = (st * 64 + (uint64_t) lane_id()) * 16;
        // the lanes of this call: g0 < hi && g0 + 16 > lo.  The step is the whole wave's and tests the second half itself; a lane
        // at or past hi gets its callbacks and drops them.
        const bool mine = g0 < hi;
        uint32_t pk[8] = {0, 0, 0, 0, 0, 0, 0, 0}, mask = 0;
        const uint32_t bad = flat_step_visit<false>(bases, offsets, n_seq, total, lo, k, st, r_hint, [&](int j, uint64_t canon, uint32_t) {
            if (!mine) return;
            uint32_t c = 0;
            if (!empty) {
                c = count_lookup(t, canon);
                c = c > maxc ? maxc : c;
            }
            pk[j >> 1] |= c << (16 * (j & 1));
            mask |= 1u << j;
        });
        if (bad && mine && g0 + 16 > lo) { // only the bytes of [lo, hi) are this call's
            const uint32_t blo = lo > g0 ? (uint32_t) (lo - g0) : 0u, bhi = hi - g0 > 16 ? 16u : (uint32_t) (hi - g0);
            anybad |= bad & ((1u << bhi) - 1u) & ~((1u << blo) - 1u);
        }
        if (!mask) continue;
        uint16_t *o = counts + (g0 - cbase);
        if (mask == 0xFFFFu && vec) {
            uint4 *o4 = reinterpret_cast<uint4 *>(o);
            o4[0] = make_uint4(pk[0], pk[1], pk[2], pk[3]);
            o4[1] = make_uint4(pk[4], pk[5], pk[6], pk[7]);
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if ((mask >> j) & 1u) o[j] = (uint16_t) (pk[j >> 1] >> (16 * (j & 1)));
        }
    }
    if (anybad) atomicOr(err, DERR_NON_ACGT);
}

// the longest sequence of a batch (device input of 2^32 bases or more: is any single read that long?)
__global__ void __launch_bounds__(256) k_profile_maxlen(const uint64_t *offsets, uint32_t n_seq, unsigned long long *out) {
    uint64_t m = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t L = offsets[i + 1] - offsets[i];
        m = L > m ? L : m;
    }
    m = wave_max_u64(m);
    if (lane_id() == 0 && m) atomicMax(out, (unsigned long long) m);
}

// ------------------------------------------------------------------------------------------------
// per-read statistics from the uint16 counts
// ------------------------------------------------------------------------------------------------
// the bin of a 256-bin histogram that holds the item of rank `rank` (ascending, rank < the histogram's total), by one whole wave;
// `below`: the items in the bins before it
__device__ __forceinline__ uint32_t wave_select256(const uint32_t *h, uint32_t rank, uint32_t &below) {
    const int lane = lane_id();
    const uint32_t b0 = h[4 * lane], b1 = h[4 * lane + 1], b2 = h[4 * lane + 2], b3 = h[4 * lane + 3];
    const uint32_t s = b0 + b1 + b2 + b3;
    const uint32_t incl = wave_incl_scan_u32(s), excl = incl - s;
    const uint64_t m = __ballot(incl > rank);
    const int src = m ? __ffsll((unsigned long long) m) - 1 : 63;
    const uint32_t q = rank - excl; // (meaningful in lane src)
    uint32_t bin, bel;
    if (q < b0) { bin = 0; bel = excl; }
    else if (q < b0 + b1) { bin = 1; bel = excl + b0; }
    else if (q < b0 + b1 + b2) { bin = 2; bel = excl + b0 + b1; }
    else { bin = 3; bel = excl + b0 + b1 + b2; }
    below = bcast_u32(bel, src);
    return bcast_u32(bin + 4u * (uint32_t) lane, src);
}

// what the waves of a block hand each other (block shape)
struct ProfShared {
    uint32_t absent, once, solid, mn, mx, bin, below, pad;
    unsigned long long sum;
};

__device__ __forceinline__ void write_abundance(kmu_read_abundance *out, uint32_t n, uint32_t absent, uint32_t once, uint32_t solid,
                                                uint32_t mn, uint32_t med, uint32_t mx, uint64_t sum) {
    out->n_kmers = n;
    out->n_absent = absent;
    out->n_once = once;
    out->n_solid = solid;
    out->min = (uint16_t) mn;
    out->median = (uint16_t) med;
    out->max = (uint16_t) mx;
    out->reserved = 0;
    out->sum = sum;
}

// The record of one read from its n counts p[0 .. n): by one wave (BLOCK = false; hist: the wave's own 256 bins) or by the whole
// block (BLOCK = true; every thread of the block calls it with the same arguments).
template <bool BLOCK>
__device__ __forceinline__ void read_stats(const uint16_t *p, uint32_t n, uint32_t solid_min, bool two_round, uint32_t *hist,
                                           ProfShared *sh, kmu_read_abundance *out) {
    const uint32_t tid = BLOCK ? threadIdx.x : (uint32_t) lane_id(), nthr = BLOCK ? 256u : 64u;
    auto sync = [] {
        if (BLOCK) __syncthreads();
        else __threadfence_block(); // one wave: its LDS operations complete in order
    };
    if (n == 0) { // shorter than k: the all-zero record
        if (tid == 0) write_abundance(out, 0, 0, 0, 0, 0, 0, 0, 0);
        return;
    }
    for (uint32_t i = tid; i < 256u; i += nthr) hist[i] = 0u;
    if (BLOCK && tid == 0) {
        sh->absent = sh->once = sh->solid = sh->mx = 0u;
        sh->mn = 0xFFFFFFFFu;
        sh->sum = 0ull;
    }
    sync();
    uint32_t absent = 0, once = 0, solid = 0, mn = 0xFFFFFFFFu, mx = 0;
    uint64_t sum = 0;
    for (uint32_t i = tid; i < n; i += nthr) {
        const uint32_t c = p[i];
        absent += c == 0u;
        once += c == 1u;
        solid += c >= solid_min;
        mn = c < mn ? c : mn;
        mx = c > mx ? c : mx;
        sum += c;
        atomicAdd(&hist[two_round ? c >> 8 : c], 1u);
    }
    absent = wave_sum_u32(absent);
    once = wave_sum_u32(once);
    solid = wave_sum_u32(solid);
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    sum = wave_sum_u64(sum);
    if (BLOCK) {
        if (lane_id() == 0) {
            atomicAdd(&sh->absent, absent);
            atomicAdd(&sh->once, once);
            atomicAdd(&sh->solid, solid);
            atomicMin(&sh->mn, mn);
            atomicMax(&sh->mx, mx);
            atomicAdd(&sh->sum, (unsigned long long) sum);
        }
    }
    sync();
    // the median: the value of rank (n - 1) / 2
    uint32_t rank = (n - 1u) / 2u, below = 0, bin = 0;
    if (!BLOCK) bin = wave_select256(hist, rank, below);
    else {
        if (threadIdx.x < 64u) {
            bin = wave_select256(hist, rank, below);
            if (tid == 0) { sh->bin = bin; sh->below = below; }
        }
        sync();
        bin = sh->bin;
        below = sh->below;
    }
    uint32_t med = bin;
    if (two_round) { // `bin` is the median's high byte: the low byte among the counts that share it
        const uint32_t hb = bin;
        sync(); // (everyone has read the round-1 histogram and sh->bin)
        for (uint32_t i = tid; i < 256u; i += nthr) hist[i] = 0u;
        sync();
        for (uint32_t i = tid; i < n; i += nthr) {
            const uint32_t c = p[i];
            if ((c >> 8) == hb) atomicAdd(&hist[c & 255u], 1u);
        }
        sync();
        rank -= below;
        if (!BLOCK) bin = wave_select256(hist, rank, below);
        else {
            if (threadIdx.x < 64u) {
                bin = wave_select256(hist, rank, below);
                if (tid == 0) sh->bin = bin;
            }
            sync();
            bin = sh->bin;
        }
        med = (hb << 8) | bin;
    }
    if (tid == 0) {
        if (BLOCK) write_abundance(out, n, sh->absent, sh->once, sh->solid, sh->mn, med, sh->mx, sh->sum);
        else write_abundance(out, n, absent, once, solid, mn, med, mx, sum);
    }
    sync(); // (block shape: sh and hist are free for the next read)
}

// reads [r0, r1): counts[offsets[r] - cbase + p] is the count at position p of read r.  A block takes tiles of 64 reads: its
// four waves take the reads of at most short_max k-mers one read per wave, then the block takes the longer ones together.
__global__ void __launch_bounds__(256) k_profile_stats(const uint16_t *counts, uint64_t cbase, const uint64_t *offsets, uint32_t r0,
                                                       uint32_t r1, int k, uint32_t solid_min, int two_round, uint32_t short_max,
                                                       kmu_read_abundance *out) {
    __shared__ uint32_t whist[4][256];
    __shared__ ProfShared sh;
    __shared__ unsigned long long longmask;
    const int wave = threadIdx.x >> 6;
    if (threadIdx.x == 0) longmask = 0ull;
    __syncthreads();
    const uint32_t ntiles = (r1 - r0 + 63u) / 64u;
    for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint32_t base = r0 + tile * 64u, cnt = r1 - base < 64u ? r1 - base : 64u;
        for (uint32_t j = wave; j < cnt; j += 4u) {
            const uint32_t r = base + j;
            const uint64_t b = offsets[r], L = offsets[r + 1] - b;
            const uint32_t n = L >= (uint64_t) k ? (uint32_t) (L - k + 1) : 0u;
            if (n > short_max) {
                if (lane_id() == 0) atomicOr(&longmask, 1ull << j);
                continue;
            }
            read_stats<false>(counts + (b - cbase), n, solid_min, two_round != 0, whist[wave], nullptr, out + r);
        }
        __syncthreads();
        unsigned long long m = longmask;
        __syncthreads();
        if (threadIdx.x == 0) longmask = 0ull;
        while (m) {
            const uint32_t j = (uint32_t) __ffsll(m) - 1u;
            m &= m - 1ull;
            const uint32_t r = base + j;
            const uint64_t b = offsets[r], L = offsets[r + 1] - b;
            read_stats<true>(counts + (b - cbase), (uint32_t) (L - k + 1), solid_min, two_round != 0, whist[0], &sh, out + r);
        }
        __syncthreads();
    }
}

// ---- a read longer than the workspace, over sub-ranges ---------------------------------------------------------------------
// acc[0] += absent, [1] += once, [2] += solid, [3] = min, [4] = max, [5] += sum; bighist[v] += counts equal to v (65536 bins)
__global__ void __launch_bounds__(256) k_profile_big_accum(const uint16_t *p, uint64_t n, uint32_t solid_min,
                                                           unsigned long long *acc, uint32_t *bighist) {
    __shared__ uint32_t lhist[256]; // the counts below 256 (nearly all of them) meet in LDS first
    lhist[threadIdx.x] = 0u;
    __syncthreads();
    uint32_t absent = 0, once = 0, solid = 0, mn = 0xFFFFFFFFu, mx = 0;
    uint64_t sum = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t c = p[i];
        absent += c == 0u;
        once += c == 1u;
        solid += c >= solid_min;
        mn = c < mn ? c : mn;
        mx = c > mx ? c : mx;
        sum += c;
        if (c < 256u) atomicAdd(&lhist[c], 1u);
        else atomicAdd(&bighist[c], 1u);
    }
    absent = wave_sum_u32(absent);
    once = wave_sum_u32(once);
    solid = wave_sum_u32(solid);
    mn = wave_min_u32(mn);
    mx = wave_max_u32(mx);
    sum = wave_sum_u64(sum);
    if (lane_id() == 0) {
        if (absent) atomicAdd(&acc[0], (unsigned long long) absent);
        if (once) atomicAdd(&acc[1], (unsigned long long) once);
        if (solid) atomicAdd(&acc[2], (unsigned long long) solid);
        atomicMin(&acc[3], (unsigned long long) mn);
        atomicMax(&acc[4], (unsigned long long) mx);
        if (sum) atomicAdd(&acc[5], (unsigned long long) sum);
    }
    __syncthreads();
    if (lhist[threadIdx.x]) atomicAdd(&bighist[threadIdx.x], lhist[threadIdx.x]);
}

// one block: the record of the read from what k_profile_big_accum gathered over its n counts
__global__ void __launch_bounds__(256) k_profile_big_finish(const unsigned long long *acc, const uint32_t *bighist, uint32_t n,
                                                            kmu_read_abundance *out) {
    __shared__ uint32_t part[256], low[256];
    __shared__ uint32_t s_hb, s_below;
    uint32_t s = 0;
    for (uint32_t i = 0; i < 256u; i++) s += bighist[threadIdx.x * 256u + i];
    part[threadIdx.x] = s;
    __syncthreads();
    uint32_t rank = (n - 1u) / 2u;
    if (threadIdx.x < 64u) {
        uint32_t below;
        const uint32_t hb = wave_select256(part, rank, below);
        if (threadIdx.x == 0) { s_hb = hb; s_below = below; }
    }
    __syncthreads();
    const uint32_t hb = s_hb;
    low[threadIdx.x] = bighist[hb * 256u + threadIdx.x];
    __syncthreads();
    if (threadIdx.x < 64u) {
        uint32_t below;
        const uint32_t lb = wave_select256(low, rank - s_below, below);
        if (threadIdx.x == 0)
            write_abundance(out, n, (uint32_t) acc[0], (uint32_t) acc[1], (uint32_t) acc[2], (uint32_t) acc[3], (hb << 8) | lb,
                            (uint32_t) acc[4], acc[5]);
    }
}

// ---- the bounded workspace: chunks of whole reads --------------------------------------------------------------------------
// Reads are taken in order; a chunk is the longest run of whole reads that ends at most `chunk` bases after the wave step its
// first read starts in; a read that does not fit alone is a chunk of its own, marked `big`.  One wave; plan[0] = chunks,
// plan[1] = 1 if more than max_ch were needed.
struct ProfChunk {
    uint64_t b, e;   // the bases [b, e) of the flat stream
    uint32_t r0, r1; // the reads [r0, r1)
    uint32_t big, pad;
};
__global__ void __launch_bounds__(64) k_profile_plan(const uint64_t *offsets, uint32_t n_seq, uint64_t chunk, uint32_t max_ch,
                                                     uint64_t *head, ProfChunk *plan) {
    const uint64_t total = offsets[n_seq];
    uint32_t r = 0, nch = 0, over = 0;
    while (r < n_seq) {
        if (nch == max_ch) { over = 1; break; }
        const uint64_t b = offsets[r], lim = (b & ~(uint64_t) 1023) + chunk;
        uint32_t r2 = lim >= total ? n_seq : wave_find_read(offsets, n_seq, lim); // reads r .. r2 - 1 end at or before lim
        const uint32_t big = r2 <= r;
        if (big) r2 = r + 1;
        if (lane_id() == 0) {
            ProfChunk c;
            c.b = b; c.e = offsets[r2]; c.r0 = r; c.r1 = r2; c.big = big; c.pad = 0;
            plan[nch] = c;
        }
        nch++;
        r = r2;
    }
    if (lane_id() == 0) { head[0] = nch; head[1] = over; }
}

static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *e = getenv(name);
    if (!e || !*e) return dflt;
    const long long v = atoll(e);
    return v > 0 ? (uint64_t) v : dflt;
}

// One wave per read up to this many k-mers, the block above (KMU_PROFILE_SHORT_MAX moves it).
static constexpr uint64_t PROFILE_SHORT_MAX = 4096;
// The counts a statistics-only call keeps at a time (2 bytes each: 256 MB; KMU_PROFILE_CHUNK moves it, tests).
static constexpr uint64_t PROFILE_CHUNK = 128ull << 20;

struct ProfileCall {
    kmu_counter *c;
    const DevSeqs *ds;
    uint32_t *d_err;
    int empty;
    uint32_t solid_min, short_max;
};

static int launch_profile(const ProfileCall &pc, uint64_t st0, uint64_t st1, uint64_t lo, uint64_t hi, uint16_t *counts, uint64_t cbase) {
    kmu_ctx *ctx = pc.c->ctx;
    if (st1 <= st0) return KMU_OK;
    const int grid = grid_for(ctx, st1 - st0, 4);
    return launch(ctx, "k_count_profile", k_count_profile, dim3(grid), dim3(256), 0, pc.ds->bases, pc.ds->offsets, pc.ds->n_seq, pc.c->p.kmer_size,
                  table_of(pc.c), pc.empty, max_count(pc.c), st0, st1, lo, hi, counts, cbase, (int) (((uintptr_t) counts & 15u) == 0), pc.d_err);
}

static int launch_stats(const ProfileCall &pc, const uint16_t *counts, uint64_t cbase, uint32_t r0, uint32_t r1, kmu_read_abundance *d_stats) {
    kmu_ctx *ctx = pc.c->ctx;
    if (r1 <= r0) return KMU_OK;
    const int grid = grid_for(ctx, r1 - r0, 64);
    return launch(ctx, "k_profile_stats", k_profile_stats, dim3(grid), dim3(256), 0, counts, cbase, pc.ds->offsets, r0, r1, pc.c->p.kmer_size,
                  pc.solid_min, (int) (max_count(pc.c) > 255u), pc.short_max, d_stats);
}

// statistics alone, the reads longer in all than the workspace: chunk by chunk
static int stats_chunked(const ProfileCall &pc, uint64_t total_bases, uint64_t chunk, kmu_read_abundance *d_stats) {
    kmu_ctx *ctx = pc.c->ctx;
    const int k = pc.c->p.kmer_size;
    const uint64_t max_ch = 2 * (total_bases / (chunk - 1023)) + 4;
    void *q;
    KMU_TRY(dev_buf(ctx, "prof.plan", 16 + (size_t) max_ch * sizeof(ProfChunk), &q));
    uint64_t *d_head = (uint64_t *) q;
    ProfChunk *d_plan = (ProfChunk *) (d_head + 2);
    KMU_TRY(launch(ctx, nullptr, k_profile_plan, dim3(1), dim3(64), 0, pc.ds->offsets, pc.ds->n_seq, chunk, (uint32_t) max_ch, d_head, d_plan));
    uint64_t head[2] = {0, 0};
    KMU_TRY(read_back(ctx, {{head, d_head, sizeof head}}));
    if (head[1] || head[0] > max_ch) return fail(ctx, KMU_E_HIP, "read profile: the chunk plan overflowed (%llu chunks)", (unsigned long long) max_ch);
    std::vector<ProfChunk> plan((size_t) head[0]);
    if (!plan.empty()) KMU_HIP(ctx, hipMemcpy(plan.data(), d_plan, plan.size() * sizeof(ProfChunk), hipMemcpyDeviceToHost));
    KMU_TRY(dev_buf(ctx, "prof.counts", ((size_t) chunk + 64) * 2, &q));
    uint16_t *ws = (uint16_t *) q;
    for (const ProfChunk &ch : plan) {
        if (!ch.big) {
            const uint64_t s0 = ch.b / 1024, s1 = (ch.e + 1023) / 1024;
            KMU_TRY(launch_profile(pc, s0, s1, ch.b, ch.e, ws, s0 * 1024));
            KMU_TRY(launch_stats(pc, ws, s0 * 1024, ch.r0, ch.r1, d_stats));
            continue;
        }
        // one read longer than the workspace: its counts pass through it a sub-range at a time
        uint32_t *qh;
        void *qa;
        KMU_TRY(dev_buf(ctx, "prof.bigacc", 64, &qa));
        KMU_TRY(dev_array(ctx, "prof.bighist", 65536, &qh));
        unsigned long long *acc = (unsigned long long *) qa;
        KMU_HIP(ctx, hipMemsetAsync(acc, 0, 64, ctx->stream));
        KMU_HIP(ctx, hipMemsetAsync(acc + 3, 0xFF, 8, ctx->stream));
        KMU_HIP(ctx, hipMemsetAsync(qh, 0, 65536 * 4, ctx->stream));
        const uint64_t pend = ch.e - k + 1; // one past the last k-mer start (a big read has more than k bases)
        const uint64_t steps = chunk / 1024;
        for (uint64_t s = ch.b / 1024; s * 1024 < pend; s += steps) {
            const uint64_t s1 = std::min(s + steps, (ch.e + 1023) / 1024);
            KMU_TRY(launch_profile(pc, s, s1, ch.b, ch.e, ws, s * 1024));
            const uint64_t p0 = std::max(ch.b, s * 1024), p1 = std::min(pend, s1 * 1024);
            KMU_TRY(launch(ctx, "k_profile_big_accum", k_profile_big_accum, dim3(grid_for(ctx, p1 - p0, 4096)), dim3(256), 0, ws + (p0 - s * 1024),
                           p1 - p0, pc.solid_min, acc, qh));
        }
        KMU_TRY(launch(ctx, "k_profile_big_finish", k_profile_big_finish, dim3(1), dim3(256), 0, acc, qh, (uint32_t) (pend - ch.b), d_stats + ch.r0));
    }
    return KMU_OK;
}

} // namespace kmu

using namespace kmu;

extern "C" {

int kmu_count_histogram(kmu_counter *c, uint64_t *hist_out, uint32_t n_bins, int mem) {
    if (!c || !hist_out || n_bins < 2 || n_bins > 65536 || (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE)) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = c->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t *d_h;
    KMU_TRY(place_output(ctx, "cnt.hist", hist_out, (size_t) n_bins, mem, &d_h));
    KMU_HIP(ctx, hipMemsetAsync(d_h, 0, (size_t) n_bins * 8, ctx->stream));
    if (!c->empty) { // (an empty counter, or one whose table waits for its first add: nothing is launched on the table)
        KMU_TRY(materialize(c));
        KMU_TRY(launch(ctx, "k_count_hist", k_count_hist, dim3(grid_for(ctx, c->nslots, 1024)), dim3(256), 0, table_of(c), c->nslots, max_count(c),
                       n_bins - 1, (unsigned long long *) d_h));
    }
    KMU_TRY(bring_output(ctx, hist_out, d_h, (size_t) n_bins, mem));
    return finish_call(ctx, mem);
}

int kmu_count_read_profile(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                           uint32_t solid_min, uint16_t *counts_out, kmu_read_abundance *stats_out) {
    if (!c || (!counts_out && !stats_out)) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = c->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (c->dist && ctx->comm && ctx->comm->nranks > 1)
        return fail(ctx, KMU_E_UNSUPPORTED, "a counter spread over %d ranks holds only its own keys: no read profile against it", ctx->comm->nranks);
    if (n_seq == 0) return KMU_OK;
    if (mem == KMU_MEM_HOST && offsets)
        for (uint32_t i = 0; i < n_seq; i++)
            if (offsets[i + 1] - offsets[i] >= (1ull << 32)) return fail(ctx, KMU_E_UNSUPPORTED, "sequence %u has 2^32 bases or more", i);
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, mem, &ds));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    uint64_t total_bases = 0;
    KMU_TRY(flat_stream_extent(ctx, offsets, n_seq, mem, ds, &total_bases));
    // device input: the walk starts `shift` bases into the caller's stream (flat_stream_extent), host input was staged re-based
    const uint64_t shift = mem == KMU_MEM_DEVICE ? (uint64_t) (ds.bases - bases) : 0;
    const uint64_t off0 = mem == KMU_MEM_HOST ? offsets[0] : 0;
    if (mem == KMU_MEM_DEVICE && total_bases >= (1ull << 32)) {
        uint64_t longest = 0;
        KMU_HIP(ctx, hipMemsetAsync(c->scalars, 0, 8, ctx->stream));
        KMU_TRY(launch(ctx, nullptr, k_profile_maxlen, dim3(grid_for(ctx, n_seq, 256)), dim3(256), 0, ds.offsets, n_seq,
                       (unsigned long long *) c->scalars));
        KMU_TRY(read_back(ctx, {{&longest, c->scalars}}));
        if (longest >= (1ull << 32)) return fail(ctx, KMU_E_UNSUPPORTED, "a sequence has 2^32 bases or more");
    }
    kmu_read_abundance *d_stats = nullptr;
    KMU_TRY(place_output(ctx, "prof.stats", stats_out, (size_t) n_seq, mem, &d_stats));
    if (total_bases == 0) { // nothing but empty sequences: no k-mer anywhere
        if (stats_out) {
            KMU_HIP(ctx, hipMemsetAsync(d_stats, 0, (size_t) n_seq * sizeof(kmu_read_abundance), ctx->stream));
            if (mem == KMU_MEM_HOST) memset(stats_out, 0, (size_t) n_seq * sizeof(kmu_read_abundance));
        }
        return finish_checked(ctx, mem, d_err);
    }
    ProfileCall pc;
    pc.c = c;
    pc.ds = &ds;
    pc.d_err = d_err;
    pc.empty = c->empty; // (nothing is launched on the table of an empty counter: every k-mer is absent)
    pc.solid_min = solid_min;
    pc.short_max = (uint32_t) std::min<uint64_t>(env_u64("KMU_PROFILE_SHORT_MAX", PROFILE_SHORT_MAX), 0xFFFFFFFFull);
    if (!pc.empty) KMU_TRY(materialize(c));
    uint64_t chunk = std::max<uint64_t>(env_u64("KMU_PROFILE_CHUNK", PROFILE_CHUNK), 2048);
    chunk = (chunk + 1023) & ~(uint64_t) 1023;
    const uint64_t nsteps = flat_wave_steps(total_bases);
    if (counts_out || total_bases <= chunk) { // every count at once: in the caller's array, its staging copy, or the workspace
        uint16_t *d_counts;
        if (counts_out && mem == KMU_MEM_DEVICE) d_counts = counts_out + shift;
        else {
            KMU_TRY(dev_array(ctx, "prof.counts", (size_t) total_bases + 64, &d_counts));
            // host arrays come back whole: the positions that start no k-mer (the last k - 1 of every sequence) as zeros
            if (counts_out) KMU_HIP(ctx, hipMemsetAsync(d_counts, 0, (size_t) total_bases * 2, ctx->stream));
        }
        KMU_TRY(launch_profile(pc, 0, nsteps, 0, ~0ull, d_counts, 0));
        if (stats_out) KMU_TRY(launch_stats(pc, d_counts, 0, 0, n_seq, d_stats));
        if (counts_out && mem == KMU_MEM_HOST)
            KMU_HIP(ctx, hipMemcpyAsync(counts_out + off0, d_counts, (size_t) total_bases * 2, hipMemcpyDeviceToHost, ctx->stream));
    } else KMU_TRY(stats_chunked(pc, total_bases, chunk, d_stats));
    KMU_TRY(bring_output(ctx, stats_out, d_stats, (size_t) n_seq, mem));
    return finish_checked(ctx, mem, d_err);
}

} // extern "C"

// kmu_count_part_kernels.hip -- the kernels of the radix-partitioned build of the count table (host side: kmu_count_part.hip;
// what the two share: kmu_count_part_kernels.h).
//
// The bases are consumed as ONE flat stream of aligned 16-byte words; the canonical k-mers travel as khash(k-mer) (kmu_count_table.h)
// and are sorted by the digits of the table's region map -- level 1 by group (the top b1 hash bits), level 2 by sub-region
// (mulhi32 of the next 32 bits with n2) -- with LDS-staged tile sorts, so that the k-mers of one bin leave as contiguous runs;
// then one workgroup per region builds the region in LDS (ds_cmpst / ds_add) and streams its image out.
#define KMU_COUNT_PART_KERNELS_TU
#include "kmu_count_part_kernels.h"
#include "kmu_flat.h"
#include "kmu_stream.h"

namespace kmu {

// level 1, pass 1 (exact route; owner census of a distributed add): per-unit histogram of the level-1 digit (also validates the bases)
__global__ void __launch_bounds__(256) k_part_hist1(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k,
                                                    PartPlan pl, uint32_t *hist1, uint32_t *err, SampleArgs sa) {
    extern __shared__ uint32_t lh[];
    const uint32_t bins1 = plan_bins1(pl);
    const Digit d1 = plan_digit1(pl);
    // sampling (owner grouping only): list and counter behind the histogram, 8-byte aligned
    uint32_t *ls_n = lh + ((bins1 + 1u) & ~1u);
    uint64_t *ls = reinterpret_cast<uint64_t *>(ls_n + 2);
    for (uint32_t b = threadIdx.x; b < bins1; b += blockDim.x) lh[b] = 0;
    if (sa.list && threadIdx.x == 0) ls_n[0] = 0;
    __syncthreads();
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t nsteps = flat_wave_steps(total);
    const uint64_t s0 = (uint64_t) blockIdx.x * pl.steps_per_unit;
    const uint64_t s1 = s0 + pl.steps_per_unit < nsteps ? s0 + pl.steps_per_unit : nsteps;
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    const uint64_t smask = sa.shift >= 32 ? 0xFFFFFFFFull : ((1ull << sa.shift) - 1ull);
    uint32_t bad = 0, r_hint = 0xFFFFFFFFu;
    // up to eight owners (one node's GPUs): a lane counts its 16 k-mers of a wave step in eight 8-bit fields of a register and
    // the wave adds its sums to the histogram with eight atomics per step (round 2 took one LDS atomic per k-mer on eight
    // addresses: 64 lanes on 8 words, 15 ms for the bench shard)
    const bool packed = pl.owner_parts != 0 && pl.owner_parts <= 8;
    for (uint64_t st = s0 + wave; st < s1; st += nwaves) {
        uint64_t pc = 0;
        bad |= flat_step_canon(bases, offsets, n_seq, total, start, k, st, r_hint, [&](uint64_t canon) {
            if (pl.owner_parts) {
                const uint64_t h = owner_hash(canon, pl.owner_w32);
                const uint32_t o = owner_of_hash(h, pl.owner_w32, pl.owner_parts);
                if (packed) pc += 1ull << (8u * o);
                else atomicAdd(&lh[o], 1u);
                if (sa.list && ((h >> 8) & smask) == 0ull) {
                    const uint32_t at = atomicAdd(&ls_n[0], 1u);
                    if (at < SAMPLE_LDS) ls[at] = canon;
                }
            } else {
                atomicAdd(&lh[digit_of_hash(d1, khash(canon))], 1u);
            }
        });
        if (packed) { // (wave-uniform) fields 0 2 4 6 and 1 3 5 7 as 16-bit numbers, two to a word: a wave's sums stay below 2^16
            const uint64_t ev = pc & 0x00FF00FF00FF00FFull, od = (pc >> 8) & 0x00FF00FF00FF00FFull;
            const uint32_t w4[4] = {(uint32_t) ev, (uint32_t) (ev >> 32), (uint32_t) od, (uint32_t) (od >> 32)};
#pragma unroll
            for (int i = 0; i < 4; i++) {
                const uint32_t sum = wave_incl_scan_u32(w4[i]); // (no carry between the halves: each stays below 2^16)
                if (lane_id() == 63) {
                    const uint32_t f0 = (uint32_t) (i & 1) * 4u + (uint32_t) (i >> 1); // owner of the low half: 0, 4, 1, 5
                    const uint32_t lo = sum & 0xFFFFu, hi = sum >> 16;
                    if (lo && f0 < bins1) atomicAdd(&lh[f0], lo);
                    if (hi && f0 + 2u < bins1) atomicAdd(&lh[f0 + 2u], hi);
                }
            }
        }
    }
    if (bad) atomicOr(err, DERR_NON_ACGT);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < bins1; b += blockDim.x) hist1[(uint64_t) blockIdx.x * bins1 + b] = lh[b];
    if (sa.list) {
        __shared__ uint32_t gbase;
        const uint32_t cnt = ls_n[0], keep = cnt < SAMPLE_LDS ? cnt : SAMPLE_LDS;
        if (threadIdx.x == 0) {
            gbase = atomicAdd(&sa.n[0], keep);
            if (cnt > SAMPLE_LDS) sa.n[1] = 1u; // the sample of this workgroup is truncated: the estimate is void
        }
        __syncthreads();
        for (uint32_t i = threadIdx.x; i < keep; i += blockDim.x)
            if (gbase + i < sa.cap) sa.list[gbase + i] = ls[i];
            else sa.n[1] = 1u;
    }
}

// distinct k-mers of the sample: every key is inserted into a scratch table (all-ones = free); a successful claim counts
__global__ void __launch_bounds__(256) k_sample_distinct(const uint64_t *list, uint32_t n, uint64_t *table, uint32_t mask,
                                                         uint32_t *n_distinct) {
    uint32_t mine = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t key = list[i];
        uint32_t off = (uint32_t) (khash(key) >> 32) & mask;
        for (uint32_t probes = 0; probes <= mask; probes++) {
            const unsigned long long old = atomicCAS((unsigned long long *) &table[off], (unsigned long long) CKEY_EMPTY, (unsigned long long) key);
            if (old == CKEY_EMPTY) { mine++; break; }
            if (old == key) break;
            off = (off + 1) & mask;
        }
    }
    if (mine) atomicAdd(n_distinct, mine);
}

// level 1 scan, step a: one workgroup per bin -> exclusive prefix over the units + bin total
__global__ void __launch_bounds__(256) k_part_scan1a(const uint32_t *hist1, PartPlan pl, uint64_t *offs1, uint64_t *tot1) {
    __shared__ uint64_t part[256];
    const uint32_t bins1 = plan_bins1(pl), b = blockIdx.x, U = pl.units1;
    const uint32_t per = (U + 255) / 256;
    const uint32_t u0 = threadIdx.x * per < U ? threadIdx.x * per : U, u1 = u0 + per < U ? u0 + per : U;
    uint64_t sum = 0;
    for (uint32_t u = u0; u < u1; u++) sum += hist1[(uint64_t) u * bins1 + b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 256; i++) { uint64_t v = part[i]; part[i] = run; run += v; }
        tot1[b] = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint32_t u = u0; u < u1; u++) {
        offs1[(uint64_t) u * bins1 + b] = run;
        run += hist1[(uint64_t) u * bins1 + b];
    }
}

// level 1 scan, step b: exclusive scan of the bin totals (single workgroup); binstart1[bins1] = number of k-mers
__global__ void __launch_bounds__(256) k_part_scan1b(const uint64_t *tot1, PartPlan pl, uint64_t *binstart1) {
    __shared__ uint64_t part[256];
    const uint32_t bins1 = plan_bins1(pl);
    const uint32_t per = (bins1 + 255) / 256;
    const uint32_t b0 = threadIdx.x * per < bins1 ? threadIdx.x * per : bins1, b1 = b0 + per < bins1 ? b0 + per : bins1;
    uint64_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += tot1[b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = 0;
        for (int i = 0; i < 256; i++) { uint64_t v = part[i]; part[i] = run; run += v; }
        binstart1[bins1] = run;
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) { binstart1[b] = run; run += tot1[b]; }
}

// ---- LDS-staged scatter -----------------------------------------------------------------------------------
// A 1024-thread workgroup sorts a tile of <= 16384 k-mers by their digit inside LDS (rank by ds_add_rtn, in-place
// exclusive scan, 8-byte staging writes) and copies the sorted tile out, so that the k-mers of one bin leave as one
// contiguous run (full sectors) instead of isolated 8-byte stores (which cost a 32-byte HBM write each: measured
// 3.7x write amplification).  The bin of a staged k-mer is recomputed from the k-mer on the way out.
__device__ __forceinline__ void vm_wait_all() { __builtin_amdgcn_s_waitcnt(0x0F70); } // vmcnt(0), expcnt / lgkmcnt untouched

struct ScatterLds {
    uint64_t *stage;  // TILE_ITEMS
    uint64_t *gbase;  // nbins: next free global position of this unit for every bin
    uint32_t *lstart; // nbins + 1: counts, then exclusive starts inside the tile
    uint32_t *wtot;   // 16 wave totals
};
__device__ __forceinline__ ScatterLds scatter_lds(uint8_t *smem, uint32_t nbins) {
    ScatterLds l;
    l.stage = reinterpret_cast<uint64_t *>(smem);
    l.gbase = l.stage + TILE_ITEMS;
    l.lstart = reinterpret_cast<uint32_t *>(l.gbase + nbins);
    l.wtot = l.lstart + nbins + 1;
    return l;
}

template <int IT>
__device__ __forceinline__ uint32_t digit_of(uint64_t item, const Digit &d) {
    if (IT == IT_OWNER) return kmer_owner(item, d.sh, d.n2);
    return digit_of_hash(d, IT == IT_HASH ? item : khash(item));
}

// it[j] == CKEY_EMPTY marks "no k-mer".  All 1024 threads call this together.  (The exact levels, the owner grouping of a
// distributed add, the generic array partition; the single-pass partition has its own form, tile_scatter_seg.)
template <int IT>
__device__ __forceinline__ void tile_scatter(uint64_t (&it)[16], const ScatterLds &l, uint32_t nbins, const Digit &d, uint64_t *out) {
    const int tid = threadIdx.x, nthreads = blockDim.x;
    uint32_t br[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        br[j] = 0;
        if (it[j] != CKEY_EMPTY) {
            uint32_t bin = digit_of<IT>(it[j], d);
            uint32_t rank = atomicAdd(&l.lstart[bin], 1u);
            br[j] = (bin << 16) | rank;
        }
    }
    lds_barrier();
    // in-place exclusive scan of lstart[0..nbins) (two bins per thread); lstart[nbins] = tile total
    {
        const uint32_t b0 = 2u * tid, b1 = b0 + 1;
        const uint32_t c0 = b0 < nbins ? l.lstart[b0] : 0u, c1 = b1 < nbins ? l.lstart[b1] : 0u;
        const uint32_t incl = wave_incl_scan_u32(c0 + c1);
        if (lane_id() == 63) l.wtot[tid >> 6] = incl;
        lds_barrier();
        uint32_t wpre = 0;
#pragma unroll
        for (int w = 0; w < 16; w++) {
            const uint32_t v = l.wtot[w];
            wpre += w < (tid >> 6) ? v : 0u;
        }
        const uint32_t excl = wpre + incl - (c0 + c1);
        if (b0 < nbins) l.lstart[b0] = excl;
        if (b1 < nbins) l.lstart[b1] = excl + c0;
        if (tid == nthreads - 1) l.lstart[nbins] = wpre + incl;
    }
    lds_barrier();
#pragma unroll
    for (int j = 0; j < 16; j++)
        if (it[j] != CKEY_EMPTY) l.stage[l.lstart[br[j] >> 16] + (br[j] & 0xFFFFu)] = it[j];
    lds_barrier();
    const uint32_t total = l.lstart[nbins];
    // eight positions at a time: the staged items, then their bins' bases, are requested together (one LDS round trip
    // per batch instead of two per position)
    for (uint32_t p0 = 0; p0 < total; p0 += 8u * nthreads) {
        uint64_t v[8], dst[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            v[u] = p < total ? l.stage[p] : CKEY_EMPTY;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            const uint32_t bin = p < total ? digit_of<IT>(v[u], d) : 0u;
            dst[u] = l.gbase[bin] + (uint64_t) (p - l.lstart[bin]);
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            if (p < total) out[dst[u]] = v[u];
        }
    }
    lds_barrier();
    uint32_t cnt[2];
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint32_t b = 2u * tid + q;
        cnt[q] = b < nbins ? l.lstart[b + 1] - l.lstart[b] : 0u;
    }
    lds_barrier();
#pragma unroll
    for (int q = 0; q < 2; q++) {
        const uint32_t b = 2u * tid + q;
        if (b < nbins) { l.gbase[b] += cnt[q]; l.lstart[b] = 0; }
    }
    if (tid == 0) l.lstart[nbins] = 0;
    lds_barrier();
}

// ---- the tile sort of the single-pass partition ------------------------------------------------------------------------
// Same tile, same runs, fewer phases: four LDS barriers per tile instead of seven and one table look-up per item on the way
// out instead of two.  The streams are SHARED by the workgroups of a set (level 1: two sets per XCD; level 2: the units of a
// level-1 bin): a tile's run of a bin is placed by an atomic add on the bin's cursor (cursor[bin]: items handed out so far), so
// the runs of the set's workgroups lie one behind the other in ONE stream per bin and the half-written 128-byte lines at the head
// of a stream are completed by the neighbours within a tile's time instead of waiting in L2 for this workgroup's next tile
// (32 workgroups x 2 048 private streams x 128 bytes = 8 MB of open lines per XCD against 4 MB of L2: the two speeds of level 1
// in round 2).  What the write-out needs is one 32-bit word per bin, grel = run start in the stream - start of the bin inside the
// tile (mod 2^32): an item at tile position p goes to slot grel[bin] + p of its stream.  The rank counters are a separate array
// that the owner zeroes while it scans them, so the ranks of the next tile are taken by the waves that are through with this
// tile's write-out while the others still store (no barrier behind the write-out).
//
// 6-byte leaf items (LEAF6): what the region build needs of an item is the 64 - w bits a slot keeps (q_kept) and it knows the
// rest from where it reads; for tables whose count field has w >= 16 bits level 2 leaves those <= 48 bits in 48-byte blocks of
// eight items (eight u32 low words, then eight u16 high parts: the two stores of an item and of its neighbours in a run land
// next to each other): 26 instead of 35 GB written and read back at the bench size.
__device__ __forceinline__ void leaf6_store(uint64_t *out, uint64_t at, uint64_t v) {
    uint8_t *b = reinterpret_cast<uint8_t *>(out) + (at >> 3) * 48u;
    reinterpret_cast<uint32_t *>(b)[at & 7u] = (uint32_t) v;
    reinterpret_cast<uint16_t *>(b + 32)[at & 7u] = (uint16_t) (v >> 32);
}
__device__ __forceinline__ uint64_t leaf6_load(const uint64_t *items, uint64_t at) {
    const uint8_t *b = reinterpret_cast<const uint8_t *>(items) + (at >> 3) * 48u;
    return ((uint64_t) reinterpret_cast<const uint16_t *>(b + 32)[at & 7u] << 32) | reinterpret_cast<const uint32_t *>(b)[at & 7u];
}
// stream (bin_base + bin) holds `cap` items at out[(bin_base + bin) * cap]; an item beyond it goes to the spill list
struct SegOut {
    uint32_t bin_base, cap;
    uint32_t *ovf;
};
struct SegLds {
    uint64_t *stage;  // TILE_ITEMS
    uint32_t *cnt;    // nbins (+ 2 pad): ranks handed out in this tile
    uint32_t *lstart; // nbins (+ 2 pad): exclusive starts inside the tile
    uint32_t *grel;   // nbins
    uint32_t *wtot;   // 16 wave totals
    uint32_t *lox;    // LEAF6: nbins -- the table's lox[] (kmu_count_table.h)
};
__device__ __forceinline__ SegLds seg_lds(uint8_t *smem, uint32_t nbins) {
    SegLds l;
    l.stage = reinterpret_cast<uint64_t *>(smem);
    l.cnt = reinterpret_cast<uint32_t *>(l.stage + TILE_ITEMS);
    l.lstart = l.cnt + nbins + 2;
    l.grel = l.lstart + nbins + 2;
    l.wtot = l.grel + nbins;
    l.lox = l.wtot + 16;
    return l;
}

// An item that finds its stream full goes to the spill list (k-mers that occur many times -- a genome at coverage c -- make
// a bin's fill vary sqrt(c) times more than the margin of independent k-mers allows for; the list is added to the finished
// table by direct insertion, k_count_add_spill); only a full spill list raises the flag that sends the batch to the exact
// levels.  ovf: [0] flag, [1] items spilled, [2] capacity of the list, [4..5] its address.
__device__ __forceinline__ void seg_spill(uint32_t *ovf, uint64_t item) {
    const uint32_t at = atomicAdd(&ovf[1], 1u);
    if (at < ovf[2]) (*reinterpret_cast<uint64_t *const *>(ovf + 4))[at] = item;
    else ovf[0] = 1u;
}

// items are khash values; nbins even, <= 2048; all 1024 threads call this together; cnt[] zero on the first call.
// MUL: the digit is the sub-region (mulhi32 of the 32 bits from bit d.sh on with d.n2: level 2, d.sh in 21 .. 31), else the group
// (the top 64 - d.sh bits: level 1).  VMWAIT: the caller prefetches the next tile with unconditional loads (see flat_step_fetch).
// ALLV: a wave whose sixteen items per lane are all k-mers (nearly every wave of long reads and of the inner levels) takes its ranks
// (bit 0) and stages its items (bit 1) without the per-item branches: the LDS requests of a lane leave back to back and are waited
// for once, not one `s_waitcnt` per item inside sixteen EXEC regions -- for the callers whose registers have the room: level 1 from
// the bases spills 25 with it and takes 18.7 instead of 12.4 ms; the array levels: 17.1 -> 16.7 ms on the bench's level 2.
template <bool VMWAIT, bool MUL, bool LEAF6, int ALLV>
__device__ __forceinline__ void tile_scatter_seg(uint64_t (&it)[16], const SegLds &l, uint32_t nbins, const Digit &d, uint64_t *out,
                                                 const SegOut &sg, uint32_t *cursor) {
    const uint32_t tid = threadIdx.x, nthreads = SCATTER_THREADS;
    const uint32_t sh = MUL ? (uint32_t) d.sh : (uint32_t) d.sh - 32u;
    auto x_of = [&](uint64_t item) -> uint32_t {
        return MUL ? __builtin_amdgcn_alignbit((uint32_t) (item >> 32), (uint32_t) item, sh) : (uint32_t) (item >> 32) >> sh;
    };
    auto bin_of = [&](uint64_t item) -> uint32_t { return MUL ? __umulhi(x_of(item), d.n2) : x_of(item); };
    uint32_t rk[8]; // ranks (< 16384), two to a register
#pragma unroll
    for (int j = 0; j < 8; j++) rk[j] = 0;
    bool allv_lane = true;
#pragma unroll
    for (int j = 0; j < 16; j++) allv_lane = allv_lane && it[j] != CKEY_EMPTY;
    const bool allv = ALLV && __all(allv_lane);
    constexpr int G = 4; // LDS round trips in flight per lane of the branch-free forms (8: 16 / 31 registers spilled)
    if ((ALLV & 1) && allv) {
#pragma unroll
        for (int h = 0; h < 16 / G; h++) {
            uint32_t r[G];
#pragma unroll
            for (int j = 0; j < G; j++) r[j] = atomicAdd(&l.cnt[bin_of(it[G * h + j])], 1u);
#pragma unroll
            for (int j = 0; j < G / 2; j++) rk[G / 2 * h + j] = r[2 * j] | (r[2 * j + 1] << 16);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (it[j] != CKEY_EMPTY) rk[j >> 1] |= atomicAdd(&l.cnt[bin_of(it[j])], 1u) << (16 * (j & 1));
    }
    lds_barrier(); // (also: every wave is through with the last tile's write-out: stage / lstart / grel are free)
    const uint32_t b0 = 2u * tid;
    uint32_t c0 = 0, c1 = 0, run0 = 0, run1 = 0;
    if (b0 < nbins) {
        const uint2 c = *reinterpret_cast<const uint2 *>(&l.cnt[b0]);
        c0 = c.x;
        c1 = c.y;
        *reinterpret_cast<uint2 *>(&l.cnt[b0]) = make_uint2(0u, 0u);
        run0 = atomicAdd(&cursor[b0], c0); // (the answers are looked at behind the staging)
        run1 = atomicAdd(&cursor[b0 + 1], c1);
    }
    const uint32_t incl = wave_incl_scan_u32(c0 + c1);
    if (lane_id() == 63) l.wtot[tid >> 6] = incl;
    lds_barrier();
    uint32_t wpre = 0, total = 0; // total: the k-mers of the tile
    {
        const uint4 *w4 = reinterpret_cast<const uint4 *>(l.wtot);
        const uint32_t wave = tid >> 6;
#pragma unroll
        for (int q = 0; q < SCATTER_THREADS / 256; q++) {
            const uint4 v = w4[q];
            const uint32_t e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int z = 0; z < 4; z++) {
                wpre += (uint32_t) (q * 4 + z) < wave ? e[z] : 0u;
                total += e[z];
            }
        }
    }
    if (b0 < nbins) {
        const uint32_t excl = wpre + incl - (c0 + c1);
        *reinterpret_cast<uint2 *>(&l.lstart[b0]) = make_uint2(excl, excl + c0);
    }
    lds_barrier();
    if ((ALLV & 2) && allv) {
#pragma unroll
        for (int h = 0; h < 16 / G; h++) {
            uint32_t at[G];
#pragma unroll
            for (int j = 0; j < G; j++) at[j] = l.lstart[bin_of(it[G * h + j])];
#pragma unroll
            for (int j = 0; j < G; j++) l.stage[at[j] + ((rk[(G * h + j) >> 1] >> (16 * (j & 1))) & 0xFFFFu)] = it[G * h + j];
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if (it[j] != CKEY_EMPTY) l.stage[l.lstart[bin_of(it[j])] + ((rk[j >> 1] >> (16 * (j & 1))) & 0xFFFFu)] = it[j];
    }
    if (b0 < nbins) {
        const uint2 ls = *reinterpret_cast<const uint2 *>(&l.lstart[b0]);
        *reinterpret_cast<uint2 *>(&l.grel[b0]) = make_uint2(run0 - ls.x, run1 - ls.y);
    }
    lds_barrier();
    if (VMWAIT) vm_wait_all(); // the next tile's requests (in flight since before the ranks) and the last tile's stores: nothing younger
    const uint32_t bb = sg.bin_base, cap = sg.cap;
    const uint64_t lowmask = (1ull << sh) - 1ull; // (LEAF6: the hash bits below x)
    for (uint32_t p0 = 0; p0 < total; p0 += 8u * nthreads) {
        uint64_t v[8];
        uint32_t rel[8], bin[8], lx[8];
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            v[u] = l.stage[p < total ? p : 0u];
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            bin[u] = bin_of(v[u]);
            rel[u] = l.grel[bin[u]] + p;
            lx[u] = LEAF6 ? l.lox[bin[u]] : 0u;
        }
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const uint32_t p = p0 + (uint32_t) u * nthreads + tid;
            if (p < total) {
                const uint64_t at = (uint64_t) (bb + bin[u]) * cap + rel[u];
                if (rel[u] >= cap) seg_spill(sg.ovf, v[u]);
                else if (LEAF6) leaf6_store(out, at, ((uint64_t) (x_of(v[u]) - lx[u]) << sh) | (v[u] & lowmask));
                else out[at] = v[u];
            }
        }
    }
}

// flat_step_load (kmu_flat.h) in two halves, for prefetching: flat_step_fetch requests the two aligned 16-byte chunks (this lane's word, the
// halo word of lane & 1) and the lane's 16 "no k-mer" bits (flat_novalid, kmu_smer.hpp), and nothing looks at them until
// flat_step_words turns them into code words one tile later -- the requests are UNCONDITIONAL loads from clamped addresses
// (needs total >= 16), so that their number in flight is a constant for the compiler's s_waitcnt placement (a load under a
// branch makes it wait for everything at the first use of anything).  All vector-memory waits of the scatter loops are the
// explicit vmcnt(0) of vm_wait_all(): once before the loop, once per tile just before the write-out, when the requests of the
// next tile have had the whole tile sort to arrive and the stores of the last tile are long gone.
struct FlatRaw {
    uint4 c0, cx;
    uint32_t nv;
};
__device__ __forceinline__ void flat_step_fetch(const uint8_t *bases, uint64_t total, uint64_t st, FlatRaw &r, const uint16_t *novalid, uint64_t last_step) {
    r.c0 = make_uint4(0u, 0u, 0u, 0u);
    r.cx = r.c0;
    r.nv = novalid[(st < last_step ? st : last_step) * 64 + (uint64_t) lane_id()];
    if (total < 16) return; // (wave-uniform; flat_step_words then reads the ragged chunk itself)
    const uint64_t lastc = (total - 16) & ~15ull;
    const uint64_t a0 = (st * 64 + (uint64_t) lane_id()) * 16, ax = (st * 64 + 64 + (uint64_t) (lane_id() & 1)) * 16;
    r.c0 = *reinterpret_cast<const uint4 *>(bases + (a0 < lastc ? a0 : lastc));
    r.cx = *reinterpret_cast<const uint4 *>(bases + (ax < lastc ? ax : lastc));
}
__device__ __forceinline__ void flat_step_words(const uint8_t *bases, uint64_t total, uint64_t st, bool active, const FlatRaw &r,
                                                uint32_t &w0, uint32_t &ex, uint32_t &bad_acc) {
    w0 = 0;
    ex = 0;
    if (!active) return; // wave-uniform
    const uint64_t i0 = st * 64 + (uint64_t) lane_id(), ix = st * 64 + 64 + (uint64_t) (lane_id() & 1);
    uint32_t bad = 0, bad2 = 0;
    if (__all(ix * 16 + 16 <= total)) { // (every chunk of the step whole: all but the last step of the stream)
        w0 = pack16_ascii(r.c0, bad);
        ex = pack16_ascii(r.cx, bad2);
    } else {
        SeqView s;
        s.base = bases; s.begin = 0; s.len = total; s.total = total; s.packed = 0;
        w0 = load_code_word(s, i0, bad);
        ex = load_code_word(s, ix, bad2);
    }
    bad_acc |= bad; // (every word is some step's own word: the halo words need no second look)
}

// up to 16 canonical k-mers of this lane for wave step `st` (CKEY_EMPTY where a k-mer would straddle a read end); the exact levels
__device__ __forceinline__ void flat_step_items(const uint64_t *offsets, uint32_t n_seq, uint64_t total, uint64_t start, int k,
                                                uint64_t st, bool active, uint32_t w0, uint32_t ex, uint32_t &r_hint, uint64_t (&it)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j++) it[j] = CKEY_EMPTY;
    if (!active) return; // wave-uniform
    // (the step keeps the reverse complement per k-mer: the exact levels' kernel has no registers for the window's)
    flat_step_visit_words<true>(offsets, n_seq, total, start, k, st, w0, ex, r_hint, [&](int j, uint64_t canon, uint32_t) { it[j] = canon; });
}

// the same from the lane's "no k-mer" bits: no read offsets, no search, no dependent look-up; a wave whose lanes are all-or-nothing
// (long reads: nearly every wave) skips the per-k-mer tests
__device__ __forceinline__ void flat_step_items_nv(int k, bool active, uint32_t w0, uint32_t ex, uint32_t nv, uint64_t (&it)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j++) it[j] = CKEY_EMPTY;
    if (!active) return; // wave-uniform
    uint32_t w1, w2;
    flat_window(w0, ex, w1, w2);
    const uint32_t V = ~nv & 0xFFFFu;
    const StepWin sw = step_win(w0, w1, w2, k);
    if (__all(V == 0xFFFFu || V == 0u)) {
        if (V) {
#pragma unroll
            for (int j = 0; j < 16; j++) it[j] = step_canonical(sw, j);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if ((V >> j) & 1u) it[j] = step_canonical(sw, j);
    }
}

// level 1, pass 2 of the exact route (private ranges per unit from the histogram), and the owner grouping of a distributed add
__global__ void __launch_bounds__(1024) k_part_scatter1_exact(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                                              int k, PartPlan pl, const uint64_t *offs1,
                                                              const uint64_t *binstart1, uint64_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t bins1 = plan_bins1(pl);
    ScatterLds l = scatter_lds(smem, bins1);
    for (uint32_t b = threadIdx.x; b < bins1; b += blockDim.x) {
        l.gbase[b] = binstart1[b] + offs1[(uint64_t) blockIdx.x * bins1 + b];
        l.lstart[b] = 0;
    }
    if (threadIdx.x == 0) l.lstart[bins1] = 0;
    lds_barrier();
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t nsteps = flat_wave_steps(total);
    const uint64_t s0 = (uint64_t) blockIdx.x * pl.steps_per_unit;
    const uint64_t s1 = s0 + pl.steps_per_unit < nsteps ? s0 + pl.steps_per_unit : nsteps;
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint32_t r_hint = 0xFFFFFFFFu, w0, ex;
    const Digit d1 = plan_digit1(pl);
    for (uint64_t t0 = s0; t0 < s1; t0 += nwaves) {
        uint64_t it[16];
        flat_step_load(bases, total, t0 + wave, t0 + wave < s1, w0, ex);
        flat_step_items(offsets, n_seq, total, start, k, t0 + wave, t0 + wave < s1, w0, ex, r_hint, it);
        if (pl.owner_parts) tile_scatter<IT_OWNER>(it, l, bins1, Digit{pl.owner_w32, pl.owner_parts}, out);
        else { // from here on the k-mers travel as their table hash
#pragma unroll
            for (int j = 0; j < 16; j++) it[j] = khash(it[j]); // (khash keeps the "no k-mer" mark)
            tile_scatter<IT_HASH>(it, l, bins1, d1, out);
        }
    }
}

// level 1 of the single-pass partition: flat base stream -> canonical k-mer -> khash -> tile sort by group -> shared streams
// [set][bin][cap] through the cursors `state`[set][bin] (set = blockIdx.x % sets: the dispatcher deals the workgroups out to the
// XCDs round robin).  The kernel validates the bases (no histogram pass ran); k_seg_tails marks the tails behind the last launch.
// Rounds (kmu_sketch_count under an upload): the same units take a slice of every round's wave steps [step_base, step_end).
__global__ void __launch_bounds__(1024) k_part_scatter1(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                                        int k, PartPlan pl, uint64_t *out, SegPlan1 seg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t bins1 = plan_bins1(pl);
    SegLds ls = seg_lds(smem, bins1);
    const uint32_t set = blockIdx.x % seg.sets;
    const SegOut sg{set * bins1, (uint32_t) seg.cap, seg.ovf};
    uint32_t *cursor = seg.state + (size_t) set * bins1;
    for (uint32_t b = threadIdx.x; b < bins1 + 2; b += blockDim.x) ls.cnt[b] = 0;
    lds_barrier();
    const uint64_t total = offsets[n_seq];
    const uint64_t nsteps_all = flat_wave_steps(total);
    const uint64_t nsteps = seg.step_end ? seg.step_end : nsteps_all;
    const uint64_t s0 = seg.step_base + (uint64_t) blockIdx.x * pl.steps_per_unit;
    const uint64_t s1 = s0 + pl.steps_per_unit < nsteps ? s0 + pl.steps_per_unit : nsteps;
    const int wave = threadIdx.x >> 6, nwaves = blockDim.x >> 6;
    uint32_t w0, ex, bad = 0;
    FlatRaw raw;
    const uint64_t last_step = nsteps_all ? nsteps_all - 1 : 0;
    flat_step_fetch(bases, total, s0 + wave, raw, seg.novalid, last_step);
    vm_wait_all();
    const Digit d1 = plan_digit1(pl);
    for (uint64_t t0 = s0; t0 < s1; t0 += nwaves) {
        uint64_t it[16];
        flat_step_words(bases, total, t0 + wave, t0 + wave < s1, raw, w0, ex, bad);
        flat_step_items_nv(k, t0 + wave < s1, w0, ex, raw.nv, it);
        // the next step's chunks and its "no k-mer" bits are requested now; they arrive under the tile sort, which waits for them
        // before its write-out
        flat_step_fetch(bases, total, t0 + nwaves + wave, raw, seg.novalid, last_step);
#pragma unroll
        for (int j = 0; j < 16; j++) it[j] = khash(it[j]); // from here on the k-mers travel as their table hash (khash keeps the "no k-mer" mark)
        tile_scatter_seg<true, false, false, 0>(it, ls, bins1, d1, out, sg, cursor);
    }
    if (bad) atomicOr(seg.err, DERR_NON_ACGT);
}

// ---- generic radix partition of a u64 array (level 2 of the read path; both levels of the array path) ------------
// The input is a set of `nparts` consecutive partitions (bounds[nparts + 1]); every partition is cut into `chunks`
// units; a unit scatters its slice by the digit `d` into `bins` sub-partitions.

__device__ __forceinline__ void arr_unit_range(const uint64_t *bounds, const ArrPlan &pl, uint32_t unit, uint64_t *i0,
                                               uint64_t *i1) {
    const uint32_t part = unit / pl.chunks, c = unit % pl.chunks;
    const uint64_t s = bounds[part], len = bounds[part + 1] - s;
    *i0 = s + len * c / pl.chunks;
    *i1 = s + len * (c + 1) / pl.chunks;
}

template <int IT>
__global__ void __launch_bounds__(256) k_arr_hist(const uint64_t *in, const uint64_t *bounds, ArrPlan pl, uint32_t *hist) {
    extern __shared__ uint32_t lh[];
    for (uint32_t b = threadIdx.x; b < pl.bins; b += blockDim.x) lh[b] = 0;
    __syncthreads();
    uint64_t i0, i1;
    arr_unit_range(bounds, pl, blockIdx.x, &i0, &i1);
    for (uint64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x)
        atomicAdd(&lh[digit_of<IT>(in[i], pl.d)], 1u);
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < pl.bins; b += blockDim.x) hist[(uint64_t) blockIdx.x * pl.bins + b] = lh[b];
}

// Offsets of the units' private output ranges; order inside a partition = (bin major, chunk minor).
// Step a: T threads share one (partition, bin): exclusive prefix of the bin's counts over the partition's chunks
// (relative offsets) and the bin total.  T = min(256, chunks) rounded down to a power of two, 256 / T bins per workgroup.
__global__ void __launch_bounds__(256) k_arr_scan_a(const uint32_t *hist, ArrPlan pl, uint32_t T, uint64_t *offs_rel,
                                                    uint64_t *tot) {
    __shared__ uint64_t part[256];
    const uint32_t bins = pl.bins, C = pl.chunks, per_wg = 256u / T;
    const uint32_t groups = (bins + per_wg - 1) / per_wg; // workgroups per partition
    const uint32_t p1 = blockIdx.x / groups, b = (blockIdx.x % groups) * per_wg + threadIdx.x / T, tc = threadIdx.x % T;
    const uint32_t per = (C + T - 1) / T;
    const uint32_t c0 = tc * per < C ? tc * per : C, c1 = c0 + per < C ? c0 + per : C;
    uint64_t sum = 0;
    if (b < bins)
        for (uint32_t c = c0; c < c1; c++) sum += hist[((uint64_t) p1 * C + c) * bins + b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (tc == 0) { // exclusive scan of this bin's T partial sums
        uint64_t run = 0;
        for (uint32_t i = 0; i < T; i++) { const uint64_t v = part[threadIdx.x + i]; part[threadIdx.x + i] = run; run += v; }
        if (b < bins) tot[(uint64_t) p1 * bins + b] = run;
    }
    __syncthreads();
    if (b < bins) {
        uint64_t run = part[threadIdx.x];
        for (uint32_t c = c0; c < c1; c++) {
            offs_rel[((uint64_t) p1 * C + c) * bins + b] = run;
            run += hist[((uint64_t) p1 * C + c) * bins + b];
        }
    }
}

// Step b: one workgroup per partition: exclusive scan of the bin totals, shifted by the partition's start ->
// outbounds[p1 * bins + b]; outbounds[nparts * bins] = end of the last partition.
__global__ void __launch_bounds__(256) k_arr_scan_b(const uint64_t *tot, const uint64_t *bounds, ArrPlan pl, uint64_t *outbounds) {
    __shared__ uint64_t part[256];
    const uint32_t bins = pl.bins, p1 = blockIdx.x;
    const uint32_t per = (bins + 255) / 256;
    const uint32_t b0 = threadIdx.x * per < bins ? threadIdx.x * per : bins, b1 = b0 + per < bins ? b0 + per : bins;
    uint64_t sum = 0;
    for (uint32_t b = b0; b < b1; b++) sum += tot[(uint64_t) p1 * bins + b];
    part[threadIdx.x] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = bounds[p1];
        for (int i = 0; i < 256; i++) { uint64_t v = part[i]; part[i] = run; run += v; }
        if (p1 == pl.nparts - 1) outbounds[(uint64_t) pl.nparts * bins] = bounds[pl.nparts];
    }
    __syncthreads();
    uint64_t run = part[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) {
        outbounds[(uint64_t) p1 * bins + b] = run;
        run += tot[(uint64_t) p1 * bins + b];
    }
}

// the exact route: unit (partition, chunk) writes bin b into its private range from the histogram
template <int IT>
__global__ void __launch_bounds__(SCATTER_THREADS) k_arr_scatter_exact(const uint64_t *in, const uint64_t *bounds, ArrPlan pl,
                                                                       const uint64_t *offs_rel, const uint64_t *outbounds, uint64_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr uint32_t TILE = 16u * SCATTER_THREADS;
    ScatterLds l = scatter_lds(smem, pl.bins);
    for (uint32_t b = threadIdx.x; b < pl.bins; b += blockDim.x) {
        l.gbase[b] = outbounds[(uint64_t) (blockIdx.x / pl.chunks) * pl.bins + b] + offs_rel[(uint64_t) blockIdx.x * pl.bins + b];
        l.lstart[b] = 0;
    }
    if (threadIdx.x == 0) l.lstart[pl.bins] = 0;
    lds_barrier();
    uint64_t i0, i1;
    arr_unit_range(bounds, pl, blockIdx.x, &i0, &i1);
    uint64_t nxt[16];
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint64_t i = i0 + (uint64_t) j * blockDim.x + threadIdx.x;
        nxt[j] = i < i1 ? in[i] : CKEY_EMPTY;
    }
    for (uint64_t t0 = i0; t0 < i1; t0 += TILE) {
        uint64_t it[16];
#pragma unroll
        for (int j = 0; j < 16; j++) it[j] = nxt[j];
        // the next tile is requested before this one is sorted: its HBM latency hides under the LDS work
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t i = t0 + TILE + (uint64_t) j * blockDim.x + threadIdx.x;
            nxt[j] = i < i1 ? in[i] : CKEY_EMPTY;
        }
        if (IT == IT_KEY_TO_HASH) { // from here on the k-mers travel as their table hash (no further evaluations)
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (it[j] != CKEY_EMPTY) it[j] = khash(it[j]);
        }
        tile_scatter<IT == IT_KEY_TO_HASH ? IT_HASH : IT>(it, l, pl.bins, pl.d, out);
    }
}

// The single-pass form: no histogram ran; "no k-mer" marks in the input (the tails of the previous level's streams) are skipped
// like everywhere else.
//  IT_HASH (level 2 of the read path and of the array path): the `chunks` units of an input partition (a level-1 bin) write ONE
//   set of leaves, a tile's run of a leaf placed by an atomic add on the leaf's cursor (leafcnt[leaf], zero before the launch; it
//   ends as the leaf's fill -- or more, where items went to the spill list: the build clamps it).  The units of a partition are the
//   workgroups 8 apart in the grid: the dispatcher deals workgroups out to the 8 XCDs round robin, so they run at the same time on
//   the same XCD and its L2 sees their runs of a leaf side by side.  The input is requested a tile ahead, whole, by unconditional
//   loads (positions beyond the partition are mapped to its last block and not looked at), the waits are explicit.
//  IT_KEY_TO_HASH (level 1 of an array of canonical k-mers): keys in, khash out, pl.out_sets sets of shared streams.
template <int IT, bool LEAF6>
__global__ void __launch_bounds__(SCATTER_THREADS) k_arr_scatter_seg(const uint64_t *in, const uint64_t *bounds, ArrPlan pl, uint64_t *out,
                                                                     uint64_t seg_cap, uint32_t *seg_ovf, uint32_t *leafcnt, const uint32_t *lox) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr uint32_t TILE = 16u * SCATTER_THREADS, THREADS = SCATTER_THREADS;
    constexpr bool L2 = IT == IT_HASH;
    SegLds ls = seg_lds(smem, pl.bins);
    uint64_t sp = blockIdx.x / pl.chunks;
    uint32_t my_chunk = blockIdx.x % pl.chunks;
    if (pl.seg_units && (pl.nparts & 7u) == 0u) {
        sp = 8u * (blockIdx.x / (8u * pl.chunks)) + (blockIdx.x & 7u);
        my_chunk = (blockIdx.x >> 3) % pl.chunks;
    }
    const uint32_t nsets = pl.out_sets > 1u ? pl.out_sets : 1u;
    const uint64_t block = sp * nsets + (nsets > 1u ? blockIdx.x % nsets : 0u);
    const SegOut sg{(uint32_t) (block * pl.bins), (uint32_t) seg_cap, seg_ovf};
    uint32_t *cursor = leafcnt + block * pl.bins;
    for (uint32_t b = threadIdx.x; b < pl.bins + 2; b += blockDim.x) ls.cnt[b] = 0;
    if (LEAF6)
        for (uint32_t b = threadIdx.x; b < pl.bins; b += blockDim.x) ls.lox[b] = lox[b];
    lds_barrier();
    uint64_t i0, i1;
    if (pl.seg_units) { // (positions in the partition's streams, one after the other): this unit's slice, from a multiple of 16 positions on
        i1 = (uint64_t) pl.seg_units * pl.seg_cap;
        const uint64_t per = ((i1 + pl.chunks - 1) / pl.chunks + 15) & ~(uint64_t) 15;
        i0 = (uint64_t) my_chunk * per < i1 ? (uint64_t) my_chunk * per : i1;
        i1 = i0 + per < i1 ? i0 + per : i1;
    } else arr_unit_range(bounds, pl, blockIdx.x, &i0, &i1);
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    uint64_t nxt[16];
    // L2: 16 bytes per lane and request -- item 2 j2 + e of a thread is element j2 * 2 THREADS + 2 tid + e of the tile (the
    // unit starts on a multiple of 16 items: stream capacities are multiples of 16)
#pragma unroll
    for (int j = 0; j < 16; j++) {
        const uint64_t i = i0 + (uint64_t) j * blockDim.x + threadIdx.x;
        if (!L2) nxt[j] = i < i1 ? in[i] : CKEY_EMPTY;
    }
    // the 16 items of this thread of the tile that starts at position t of the partition
    const uint64_t seg_stride = (uint64_t) pl.seg_bins * pl.seg_cap, seg_base = (uint64_t) sp * pl.seg_cap;
    auto tile_request = [&](uint64_t t) {
        // position -> (block, offset); a pair of items never straddles streams (their sizes are multiples of 16)
        uint32_t i = (uint32_t) t + 2u * threadIdx.x;
        uint32_t u = i / pl.seg_cap, o = i - u * pl.seg_cap;
#pragma unroll
        for (int j2 = 0; j2 < 8; j2++) {
            // a pair beyond the unit's slice is not looked at: its lanes ask for the partition's first pair, one line that the
            // vector cache holds (requested as whole tiles a unit of 8.3 tiles fetched 10: 42.7 GB for the bench's 35.6)
            const bool mine = t + (uint64_t) j2 * (2u * THREADS) + 2u * threadIdx.x < i1;
            const u64x2 q = *reinterpret_cast<const u64x2 *>(in + (mine ? (uint64_t) u * seg_stride + seg_base + o : seg_base));
            nxt[2 * j2] = q.x;
            nxt[2 * j2 + 1] = q.y;
            o += 2u * THREADS;
            if (pl.seg_cap >= 2u * THREADS) { if (o >= pl.seg_cap) { o -= pl.seg_cap; u++; } }
            else { const uint32_t dd = o / pl.seg_cap; u += dd; o -= dd * pl.seg_cap; }
        }
    };
    if (L2) {
        if (i0 < i1) tile_request(i0);
        else {
#pragma unroll
            for (int j = 0; j < 16; j++) nxt[j] = CKEY_EMPTY;
        }
        vm_wait_all();
    }
    for (uint64_t t0 = i0; t0 < i1; t0 += TILE) {
        uint64_t it[16];
#pragma unroll
        for (int j = 0; j < 16; j++) {
            if (L2) it[j] = t0 + (uint64_t) (j >> 1) * (2u * THREADS) + 2u * threadIdx.x + (j & 1) < i1 ? nxt[j] : CKEY_EMPTY;
            else it[j] = nxt[j];
        }
        // the next tile is requested before this one is sorted: its HBM latency hides under the LDS work
        if (L2) tile_request(t0 + TILE);
        else {
#pragma unroll
            for (int j = 0; j < 16; j++) {
                const uint64_t i = t0 + TILE + (uint64_t) j * blockDim.x + threadIdx.x;
                nxt[j] = i < i1 ? in[i] : CKEY_EMPTY;
            }
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (it[j] != CKEY_EMPTY) it[j] = khash(it[j]); // from here on the k-mers travel as their table hash
        }
        tile_scatter_seg<L2, L2, LEAF6, 3>(it, ls, pl.bins, pl.d, out, sg, cursor);
    }
}

// Level 1 of the receiver of a super-k-mer exchange (kmu_smer.h): the input is an array of 12-byte records, a thread takes one
// record per tile and expands it into its <= 16 canonical k-mers with the window arithmetic of the read path (a record IS the
// lane's three code words); from there on the tile sort of the single-pass partition, shared streams and cursors as in
// k_arr_scatter_seg<IT_KEY_TO_HASH>.  Unit u of `chunks` takes records [n u / chunks, n (u + 1) / chunks).
__global__ void __launch_bounds__(SCATTER_THREADS) k_smer_scatter1(const uint32_t *recs, uint64_t n_rec, int k, ArrPlan pl, uint64_t *out,
                                                                  uint64_t seg_cap, uint32_t *seg_ovf, uint32_t *cursors) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    SegLds ls = seg_lds(smem, pl.bins);
    const uint32_t nsets = pl.out_sets > 1u ? pl.out_sets : 1u;
    const uint32_t block = nsets > 1u ? blockIdx.x % nsets : 0u;
    const SegOut sg{block * pl.bins, (uint32_t) seg_cap, seg_ovf};
    uint32_t *cursor = cursors + (size_t) block * pl.bins;
    for (uint32_t b = threadIdx.x; b < pl.bins + 2; b += blockDim.x) ls.cnt[b] = 0;
    lds_barrier();
    const uint64_t i0 = n_rec * blockIdx.x / pl.chunks, i1 = n_rec * (blockIdx.x + 1) / pl.chunks;
    uint32_t nx0 = 0, nx1 = 0, nx2 = 0;
    bool nxv = false;
    auto fetch = [&](uint64_t i) {
        nxv = i < i1;
        if (nxv) { nx0 = recs[i * 3]; nx1 = recs[i * 3 + 1]; nx2 = recs[i * 3 + 2]; }
    };
    fetch(i0 + threadIdx.x);
    for (uint64_t t0 = i0; t0 < i1; t0 += SCATTER_THREADS) {
        const uint32_t w0 = nx0, w1 = nx1, w2 = nx2, L = nxv ? (nx2 & 15u) + 1u : 0u;
        fetch(t0 + SCATTER_THREADS + threadIdx.x); // the next tile's record arrives under this tile's sort
        uint64_t it[16];
        const StepWin sw = step_win(w0, w1, w2 & ~15u, k); // (the low four bits of a record's last word: its k-mer count)
#pragma unroll
        for (int j = 0; j < 16; j++)
            it[j] = (uint32_t) j < L ? khash(step_canonical(sw, j)) : CKEY_EMPTY; // kmer.reverse_complement().min(kmer), kmercount.rs:938
        tile_scatter_seg<false, false, false, 0>(it, ls, pl.bins, pl.d, out, sg, cursor);
    }
}

// the overflow word block of a single-pass partition (seg_spill): flag and count zero, capacity and address of the list
__global__ void __launch_bounds__(64) k_spill_header(uint32_t *ovf, uint32_t cap, uint64_t *list) {
    if (threadIdx.x < 16) ovf[threadIdx.x] = 0u;
    __syncthreads();
    if (threadIdx.x == 0) {
        ovf[2] = cap;
        *reinterpret_cast<uint64_t **>(ovf + 4) = list;
    }
}

// "no k-mer" marks from the fill of every (set, bin) stream of level 1 to its capacity (level 2 reads whole streams)
// (a few workgroups per CU, each over many streams, 16 bytes per lane: one workgroup per stream -- 32 768 launches of 15 KB at the
//  bench size -- took 0.7 ms for 0.5 GB)
__global__ void __launch_bounds__(256) k_seg_tails(const uint32_t *cursor, uint32_t n_streams, uint32_t cap, uint64_t *out) {
    typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
    for (uint32_t s = blockIdx.x; s < n_streams; s += gridDim.x) {
        uint32_t n = cursor[s] < cap ? cursor[s] : cap;
        uint64_t *o = out + (uint64_t) s * cap;
        if ((n & 1u) && n < cap) { // (cap is even: pairs from an even position on)
            if (threadIdx.x == 0) o[n] = CKEY_EMPTY;
            n++;
        }
        for (uint32_t i = n + 2u * threadIdx.x; i < cap; i += 2u * blockDim.x) *reinterpret_cast<u64x2 *>(o + i) = u64x2{CKEY_EMPTY, CKEY_EMPTY};
    }
}

// the spill list of a single-pass partition (khash values) into the finished table, by direct insertion
__global__ void __launch_bounds__(256) k_count_add_spill(const uint64_t *items, const uint32_t *ovf, CountTable t, uint32_t *err) {
    const uint32_t n = ovf[1] < ovf[2] ? ovf[1] : ovf[2];
    bool full = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!count_insert_h(t, t.w ? 0ull : khash_inv(items[i]), items[i], 1u)) full = true;
    if (full) atomicOr(err, DERR_TABLE_FULL);
}

// out[i] = i * stride
__global__ void __launch_bounds__(256) k_fill_linear(uint64_t *out, uint64_t n, uint64_t stride) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) out[i] = i * stride;
}

// ---- the region build: one workgroup per region --------------------------------------------------------------------------
// The region lives in LDS while its k-mers are inserted, then it leaves for HBM.  in_mode: 0 = the table holds nothing yet (no
// region is read), 1 = the slab is read first.  The first BUILD_PRE items of every thread are requested before the region is
// initialised, so their HBM latency hides under the LDS fill; the workgroups of a CU overlap each other's phases.

// where the items of region r lie: [leafstart[r], leafstart[r + 1]) (exact route), or a fixed-size leaf with its fill in leafcnt
// (single-pass route: the fill may exceed the capacity where items went to the spill list)
__device__ __forceinline__ void leaf_range(uint32_t r, const uint64_t *leafstart, uint64_t leaf_stride, const uint32_t *leafcnt, uint64_t &i0, uint64_t &i1) {
    if (leaf_stride) {
        i0 = (uint64_t) r * leaf_stride;
        i1 = i0 + (leafcnt[r] < leaf_stride ? (uint64_t) leafcnt[r] : leaf_stride);
    } else {
        i0 = leafstart ? leafstart[r] : 0;
        i1 = leafstart ? leafstart[r + 1] : 0;
    }
}

// Quotient slots: the region is 4 096 8-byte words in LDS (32 KiB: four workgroups of 512 threads per CU), a first sighting is
// one ds_cmpst_rtn_b64, a repeat one more ds_add_u64 (guarded: the count field stops short of its width), and the LDS image leaves as
// it is.  LEAF6: the leaves hold the <= 48 bits a slot keeps of an item (tile_scatter_seg) instead of its hash.
// The items of a workgroup's NEXT region are requested before this region is built, and the bounds of the one after that with
// them (round 5): a leaf's items come from HBM at the latency of a memory system that the builds themselves keep busy, and a
// workgroup that asks at the top of its region (first for the leaf's fill, then for the items) waits for them behind the LDS fill
// with only the three other workgroups of its CU to cover for it.
template <int IT, bool LEAF6>
__global__ void __launch_bounds__(BUILD_THREADS, 8) k_part_build_q(const uint64_t *__restrict__ items, const uint64_t *__restrict__ leafstart,
                                                                uint32_t n_regions, CountTable t, int in_mode, uint32_t *err,
                                                                uint64_t leaf_stride, const uint32_t *__restrict__ leafcnt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t R = t.rmask + 1;
    uint64_t *lk = reinterpret_cast<uint64_t *>(smem);
    uint4 *lk4 = reinterpret_cast<uint4 *>(lk);
    const uint32_t tid = threadIdx.x;
    uint64_t *pool = lk + R + (uint32_t) __builtin_amdgcn_readfirstlane((int) (tid >> 6)) * BUILD_POOL; // this wave's
    uint32_t full = 0;
    const int w = t.w, xs = 32 - t.b1, os = 32 - t.rbits;
    const uint64_t cmask = q_cmask(w), lowmask = (1ull << xs) - 1ull;
    const uint64_t add_limit = q_limit(w);
    auto item_at = [&](uint64_t i) -> uint64_t { return LEAF6 ? leaf6_load(items, i) : items[i]; };
    // where the items of region rr lie (nothing for a region beyond the table), and the first BUILD_PRE of them of this thread
    auto range = [&](uint32_t rr, uint64_t &a0, uint64_t &a1) {
        a0 = a1 = 0;
        if (rr < n_regions) leaf_range(rr, leafstart, leaf_stride, leafcnt, a0, a1);
    };
    // the requested items wait a region long in registers: as nine words where they are 48-bit leaves (twelve otherwise)
    struct Ahead {
        uint32_t lo[BUILD_PRE], hi[LEAF6 ? BUILD_PRE / 2 : BUILD_PRE];
    };
    auto request = [&](uint64_t a0, uint64_t a1, Ahead &it) {
#pragma unroll
        for (int q = 0; q < BUILD_PRE; q++) {
            const uint64_t i = a0 + (uint64_t) q * BUILD_THREADS + tid;
            if (LEAF6) {
                const uint8_t *b = reinterpret_cast<const uint8_t *>(items) + (i >> 3) * 48u;
                it.lo[q] = i < a1 ? reinterpret_cast<const uint32_t *>(b)[i & 7u] : ~0u;
                const uint32_t h = i < a1 ? (uint32_t) reinterpret_cast<const uint16_t *>(b + 32)[i & 7u] : 0xFFFFu;
                it.hi[q >> 1] = (q & 1) ? it.hi[q >> 1] | (h << 16) : h;
            } else {
                const uint64_t v = i < a1 ? items[i] : CKEY_EMPTY;
                it.lo[q] = (uint32_t) v;
                it.hi[q] = (uint32_t) (v >> 32);
            }
        }
    };
    // (a 48-bit leaf item is never all ones: the "no item" mark of a lane beyond the leaf's fill is 2^48 - 1)
    auto unpack = [&](const Ahead &it, int q) -> uint64_t {
        if (!LEAF6) return ((uint64_t) it.hi[q] << 32) | it.lo[q];
        const uint64_t v = ((uint64_t) ((it.hi[q >> 1] >> (16 * (q & 1))) & 0xFFFFu) << 32) | it.lo[q];
        return v == 0xFFFFFFFFFFFFull ? CKEY_EMPTY : v;
    };
    Ahead nxt_it;
    uint64_t n0 = 0, n1 = 0, m0 = 0, m1 = 0;
    range(blockIdx.x, n0, n1);
    request(n0, n1, nxt_it);
    range(blockIdx.x + gridDim.x, m0, m1);
    if (in_mode != 1) {
        for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) lk4[s] = make_uint4(~0u, ~0u, ~0u, ~0u);
        lds_barrier();
    }
    for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
        uint64_t pre_it[BUILD_PRE];
        const uint64_t i0 = n0, i1 = n1;
#pragma unroll
        for (int q = 0; q < BUILD_PRE; q++) pre_it[q] = unpack(nxt_it, q);
        n0 = m0;
        n1 = m1;
        request(n0, n1, nxt_it);                 // region r + grid: its bounds have been here since the last turn
        range(r + 2u * gridDim.x, m0, m1);       // region r + 2 grid: looked at in the next turn
        const uint32_t lox_s = t.lox[r % t.n2]; // (workgroup-uniform: the sub-region of this region)
        uint4 *gk4 = reinterpret_cast<uint4 *>(t.keys + (uint64_t) r * R);
        if (in_mode == 1) { // (an empty table: the region in LDS is empty already -- the copy-out of the last one left it so)
            for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) lk4[s] = gk4[s];
            lds_barrier();
        }
        // an item -> the slot word it would claim (count 0) and its home slot
        auto locate = [&](uint64_t item, uint64_t &hw, uint32_t &off) {
            if (LEAF6) {
                const uint32_t x = lox_s + (uint32_t) (item >> xs);
                off = (x * t.n2) >> os;
                hw = item << w;
            } else {
                const uint64_t h = IT == IT_HASH ? item : khash(item);
                const uint32_t x = (uint32_t) (h >> xs);
                off = (x * t.n2) >> os;
                hw = (((uint64_t) (x - lox_s) << xs) | (h & lowmask)) << w;
            }
        };
        // one probe of `item` at slot `off`: true = the item is in (claimed a free slot, or met its own key)
        auto probe = [&](uint64_t hw, uint32_t off) -> bool {
            const unsigned long long old = atomicCAS((unsigned long long *) &lk[off], (unsigned long long) CKEY_EMPTY, (unsigned long long) (hw | 1ull));
            if (old == CKEY_EMPTY) return true;
            if (!q_same(old, hw, w)) return false;
            // the adds in flight behind a count seen below the limit are fewer than the margin: no carry into the key bits
            if ((old & cmask) < add_limit) atomicAdd((unsigned long long *) &lk[off], 1ull);
            return true;
        };
        // the rest of an item's probe sequence from its n-th probe at `off` on
        auto walk = [&](uint64_t hw, uint32_t off, uint32_t n) {
            do {
                off = (off + ++n) & t.rmask;
                if (n >= R) { full = 1; break; }
            } while (!probe(hw, off));
        };
        {
            // Item by item (rounds 2-4: every lane walking through its six items at its own pace) a wave repeats "probe, wait for the
            // answer, branch" until the unluckiest of its lanes is through -- ~31 trips of ~55 instructions where the average item
            // needs 1.6 probes; 21.3 ms for the bench's table where this form takes 20.3 (9.4 -> 7.2e9 vector, 8.2 -> 5.6e9 scalar
            // wave-instructions).  Here the first
            // probes of a thread's six items leave back to back without a branch (a lane without an item compares against 0, which no
            // slot holds, so nothing is written) and are waited for once; so do the second probes (the next slot) of the items that
            // failed; what is left -- one item in seven -- is pooled per WAVE in LDS and the lanes take the pool's entries, one each:
            // the walk of the remaining probe sequences is as long as the longest of them, not as the unluckiest lane's sum.
            // Two items at a time: a thread that has seen counts below the ceiling has at most two adds in flight behind them, the 512
            // threads 1024 = Q_MARGIN -- a field stops at 2^w - 1 at the latest, as with the item-by-item loop.
            constexpr int H = 2;
            static_assert(BUILD_THREADS * H <= (int) Q_MARGIN && BUILD_PRE % H == 0, "adds in flight against the margin of a count field");
            uint32_t n_pool = 0; // (wave-uniform)
#pragma unroll
            for (int h = 0; h < BUILD_PRE / H; h++) {
                uint64_t hw[H];
                uint32_t off[H];
                bool todo[H];
#pragma unroll
                for (int q = 0; q < H; q++) {
                    locate(pre_it[H * h + q], hw[q], off[q]);
                    todo[q] = pre_it[H * h + q] != CKEY_EMPTY;
                }
#pragma unroll
                for (int pass = 0; pass < BUILD_PASSES; pass++) {
                    unsigned long long old[H];
#pragma unroll
                    for (int q = 0; q < H; q++) {
                        if (pass == 0) // (nearly every lane has an item)
                            old[q] = atomicCAS((unsigned long long *) &lk[off[q]], todo[q] ? (unsigned long long) CKEY_EMPTY : 0ull, (unsigned long long) (hw[q] | 1ull));
                        else {         // (one lane in three)
                            off[q] = (off[q] + (uint32_t) pass) & t.rmask;
                            old[q] = 0ull;
                            if (todo[q]) old[q] = atomicCAS((unsigned long long *) &lk[off[q]], (unsigned long long) CKEY_EMPTY, (unsigned long long) (hw[q] | 1ull));
                        }
                    }
#pragma unroll
                    for (int q = 0; q < H; q++) {
                        const bool claimed = old[q] == CKEY_EMPTY, same = !claimed && q_same(old[q], hw[q], w);
                        if (todo[q] && same && (old[q] & cmask) < add_limit) atomicAdd((unsigned long long *) &lk[off[q]], 1ull);
                        todo[q] = todo[q] && !claimed && !same;
                    }
                }
#pragma unroll
                for (int q = 0; q < H; q++) {
                    const uint64_t m = __ballot(todo[q]);
                    const uint32_t at = n_pool + __builtin_amdgcn_mbcnt_hi((uint32_t) (m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t) m, 0u));
                    if (todo[q]) {
                        if (at < BUILD_POOL) pool[at] = hw[q];
                        else walk(hw[q], off[q], BUILD_PASSES - 1u); // (a wave with more than 96 of 384 items left after the batched probes: a table that is filling up)
                    }
                    n_pool += (uint32_t) __popcll(m);
                }
            }
            n_pool = n_pool < BUILD_POOL ? n_pool : BUILD_POOL;
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            for (uint32_t e = tid & 63u; e < n_pool; e += 64u) {
                const uint64_t h = pool[e];
                const uint32_t x = lox_s + (uint32_t) ((h >> w) >> xs);
                walk(h, (((x * t.n2) >> os) + (BUILD_PASSES - 1u) * BUILD_PASSES / 2u) & t.rmask, BUILD_PASSES - 1u); // (its last probe: the triangular number)
            }
            __builtin_amdgcn_wave_barrier(); // (the pool is this wave's alone: the next region's entries come behind two workgroup barriers)
        }
        for (uint64_t i = i0 + (uint64_t) BUILD_PRE * BUILD_THREADS + tid; i < i1; i += BUILD_THREADS) { // (leaves beyond 3 072 items)
            const uint64_t item = item_at(i);
            if (item == CKEY_EMPTY) continue;
            uint64_t hw;
            uint32_t off;
            locate(item, hw, off);
            if (!probe(hw, off)) walk(hw, off, 0u);
        }
        lds_barrier();
        for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) {
            gk4[s] = lk4[s];
            if (in_mode != 1) lk4[s] = make_uint4(~0u, ~0u, ~0u, ~0u);
        }
        lds_barrier();
    }
    if (full) atomicOr(err, DERR_TABLE_FULL);
}

// wide slots: keys + counts of the region in LDS (48 KiB: three workgroups per CU)
template <int IT>
__global__ void __launch_bounds__(BUILD_THREADS) k_part_build(const uint64_t *__restrict__ items, const uint64_t *__restrict__ leafstart,
                                                              uint32_t n_regions, CountTable t, int in_mode, uint32_t *err,
                                                              uint64_t leaf_stride, const uint32_t *__restrict__ leafcnt) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t R = t.rmask + 1; // >= 1024
    uint64_t *lk = reinterpret_cast<uint64_t *>(smem);
    uint32_t *lc = reinterpret_cast<uint32_t *>(lk + R);
    uint4 *lk4 = reinterpret_cast<uint4 *>(lk), *lc4 = reinterpret_cast<uint4 *>(lc);
    const uint32_t tid = threadIdx.x;
    const int xs = 32 - t.b1, os = 32 - t.rbits;
    uint32_t full = 0;
    for (uint32_t r = blockIdx.x; r < n_regions; r += gridDim.x) {
        const uint64_t gbase = (uint64_t) r * R;
        uint64_t i0, i1;
        leaf_range(r, leafstart, leaf_stride, leafcnt, i0, i1);
        uint64_t pre_it[BUILD_PRE];
#pragma unroll
        for (int q = 0; q < BUILD_PRE; q++) {
            const uint64_t i = i0 + (uint64_t) q * BUILD_THREADS + tid;
            pre_it[q] = i < i1 ? items[i] : CKEY_EMPTY;
        }
        uint4 *gk4 = reinterpret_cast<uint4 *>(t.keys + gbase), *gc4 = reinterpret_cast<uint4 *>(t.counts + gbase);
        if (in_mode == 1) {
            for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) lk4[s] = gk4[s];
            for (uint32_t s = tid; s < R / 4; s += BUILD_THREADS) lc4[s] = gc4[s];
        } else {
            for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) lk4[s] = make_uint4(~0u, ~0u, ~0u, ~0u);
            for (uint32_t s = tid; s < R / 4; s += BUILD_THREADS) lc4[s] = make_uint4(0u, 0u, 0u, 0u);
        }
        lds_barrier();
        auto insert = [&](uint64_t item) {
            const uint64_t v = IT == IT_HASH ? khash_inv(item) : item, h = IT == IT_HASH ? item : khash(item);
            uint32_t off = ((uint32_t) (h >> xs) * t.n2) >> os;
            bool done = false;
            for (uint32_t probes = 0; probes < R; probes++) {
                unsigned long long old = atomicCAS((unsigned long long *) &lk[off], (unsigned long long) CKEY_EMPTY, (unsigned long long) v);
                if (old == CKEY_EMPTY || old == v) {
                    atomicAdd(&lc[off], 1u);
                    done = true;
                    break;
                }
                off = (off + probes + 1u) & t.rmask;
            }
            if (!done) full = 1;
        };
#pragma unroll
        for (int q = 0; q < BUILD_PRE; q++)
            if (pre_it[q] != CKEY_EMPTY) insert(pre_it[q]);
        for (uint64_t i = i0 + (uint64_t) BUILD_PRE * BUILD_THREADS + tid; i < i1; i += BUILD_THREADS) {
            const uint64_t item = items[i];
            if (item != CKEY_EMPTY) insert(item);
        }
        lds_barrier();
        for (uint32_t s = tid; s < R / 2; s += BUILD_THREADS) gk4[s] = lk4[s];
        for (uint32_t s = tid; s < R / 4; s += BUILD_THREADS) gc4[s] = lc4[s];
        lds_barrier();
    }
    if (full) atomicOr(err, DERR_TABLE_FULL);
}

// the forms the host side launches (kmu_count_part_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__;
KMU_COUNT_PART_KERNEL_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

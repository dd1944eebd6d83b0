// kmu_count_part_steps.h -- the device steps that two or more of the kernel files of the partitioned build share (kmu_count_part_level1.hip,
// kmu_count_part_array.hip, kmu_count_part_build.hip; nobody else includes this): the two LDS-staged tile sorts with their LDS maps and
// prologues, the item -> digit rule, the 6-byte leaf item, the spill list, the serial scan of 256 partial sums.
#pragma once

#include "kmu_count_part_kernels.h"

namespace kmu {

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
// the prologue of a unit that writes private ranges (the exact route): first(b) = the unit's first global position of bin b, from the
// histogram's offsets; the tile's counters zero
template <typename F>
__device__ __forceinline__ void scatter_open(const ScatterLds &l, uint32_t nbins, F &&first) {
    for (uint32_t b = threadIdx.x; b < nbins; b += blockDim.x) {
        l.gbase[b] = first(b);
        l.lstart[b] = 0;
    }
    if (threadIdx.x == 0) l.lstart[nbins] = 0;
    lds_barrier();
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
// the prologue of a unit that writes shared streams: block `block` of nbins streams (a set of level 1) -> where its streams lie (sg) and
// their cursors (cursors[block][bin]); the rank counters zero.  (k_arr_scatter_seg keeps its own spelling: DESIGN 3.4)
__device__ __forceinline__ void seg_open(const SegLds &l, uint32_t nbins, uint32_t block, uint64_t cap, uint32_t *ovf, uint32_t *cursors, SegOut &sg,
                                         uint32_t *&cursor) {
    sg = SegOut{block * nbins, (uint32_t) cap, ovf};
    cursor = cursors + (size_t) block * nbins;
    for (uint32_t b = threadIdx.x; b < nbins + 2; b += blockDim.x) l.cnt[b] = 0;
    lds_barrier();
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

// ---- the scans between a histogram and its scatter -------------------------------------------------------------------------------
// 256 partial sums in LDS (part[tid], written by the caller) -> their exclusive prefix: thread 0 scans them serially from first() on and
// hands the total to total(sum) before anybody goes on; every thread then resumes from part[its own].  All 256 threads call.
template <typename F0, typename F>
__device__ __forceinline__ void block_scan_256(uint64_t *part, F0 &&first, F &&total) {
    __syncthreads();
    if (threadIdx.x == 0) {
        uint64_t run = first();
        for (int i = 0; i < 256; i++) { uint64_t v = part[i]; part[i] = run; run += v; }
        total(run);
    }
    __syncthreads();
}

} // namespace kmu

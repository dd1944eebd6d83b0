// kmu_count_part_array.hip -- the radix partition of a u64 array (level 2 of the read path; both levels of the array path; level 1 of the
// receiver of a super-k-mer exchange) and the small kernels around the shared streams (host side: kmu_count_part.hip; declarations, plans
// and constants: kmu_count_part_kernels.h; the tile sorts and the other steps shared with the kernels that walk reads: kmu_count_part_steps.h).
//
// Level 2 sorts the khash values of a level-1 bin by sub-region (mulhi32 of the next 32 hash bits with n2) into the leaves that the region
// build (kmu_count_part_build.hip) reads.
#include "kmu_count_part_steps.h"

namespace kmu {

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
    block_scan_256(part, [=] { return bounds[p1]; }, [=](uint64_t) {
        if (p1 == pl.nparts - 1) outbounds[(uint64_t) pl.nparts * bins] = bounds[pl.nparts];
    });
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
    scatter_open(l, pl.bins, [&](uint32_t b) {
        return outbounds[(uint64_t) (blockIdx.x / pl.chunks) * pl.bins + b] + offs_rel[(uint64_t) blockIdx.x * pl.bins + b];
    });
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
    // (the shared-stream prologue -- seg_open, kmu_count_part_steps.h -- stays spelled out in this kernel: through the helper the compiler
    //  lays the kernel's blocks out differently, and the instruction stream of level 2 is to stay what it was -- DESIGN 3.4)
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
    SegOut sg;
    uint32_t *cursor;
    const uint32_t nsets = pl.out_sets > 1u ? pl.out_sets : 1u;
    seg_open(ls, pl.bins, nsets > 1u ? blockIdx.x % nsets : 0u, seg_cap, seg_ovf, cursors, sg, cursor);
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

// out[i] = i * stride
__global__ void __launch_bounds__(256) k_fill_linear(uint64_t *out, uint64_t n, uint64_t stride) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) out[i] = i * stride;
}

// the forms the host side launches (kmu_count_part_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__;
KMU_COUNT_PART_ARRAY_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

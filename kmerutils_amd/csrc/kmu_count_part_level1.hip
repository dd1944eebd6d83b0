// kmu_count_part_level1.hip -- the kernels of the partitioned build that walk reads (host side: kmu_count_part.hip; declarations, plans and
// constants: kmu_count_part_kernels.h; the steps shared with the other kernel files: kmu_count_part_steps.h).
//
// The bases are consumed as ONE flat stream of aligned 16-byte words (kmu_flat.h); the canonical k-mers travel as khash(k-mer)
// (kmu_count_table.h) and are sorted by the level-1 digit of the table's region map -- the group, the top b1 hash bits -- with an LDS-staged
// tile sort, so that the k-mers of one bin leave as contiguous runs.  Level 2 and the array levels: kmu_count_part_array.hip; the region
// build: kmu_count_part_build.hip.
#include "kmu_count_part_steps.h"
#include "kmu_flat.h"

namespace kmu {

// a unit's range of wave steps [s0, s1) of the nsteps of a stream -- `steps_per_unit` from `first` + blockIdx.x * steps_per_unit on -- and
// how its waves share them: wave `wave` of `nwaves` takes every nwaves-th step
struct UnitSteps {
    uint64_t s0, s1;
    int wave, nwaves;
};
__device__ __forceinline__ UnitSteps unit_steps(uint64_t first, uint32_t steps_per_unit, uint64_t nsteps) {
    UnitSteps u;
    u.s0 = first + (uint64_t) blockIdx.x * steps_per_unit;
    u.s1 = u.s0 + steps_per_unit < nsteps ? u.s0 + steps_per_unit : nsteps;
    u.wave = threadIdx.x >> 6;
    u.nwaves = blockDim.x >> 6;
    return u;
}

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
    const UnitSteps u = unit_steps(0, pl.steps_per_unit, flat_wave_steps(total));
    const uint64_t smask = sa.shift >= 32 ? 0xFFFFFFFFull : ((1ull << sa.shift) - 1ull);
    uint32_t bad = 0, r_hint = 0xFFFFFFFFu;
    // up to eight owners (one node's GPUs): a lane counts its 16 k-mers of a wave step in eight 8-bit fields of a register and
    // the wave adds its sums to the histogram with eight atomics per step (round 2 took one LDS atomic per k-mer on eight
    // addresses: 64 lanes on 8 words, 15 ms for the bench shard)
    const bool packed = pl.owner_parts != 0 && pl.owner_parts <= 8;
    for (uint64_t st = u.s0 + u.wave; st < u.s1; st += u.nwaves) {
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
        if (packed) { // (wave-uniform) the fields as 16-bit numbers, two to a word (spread8, kmu_smer.h): a wave's sums stay below 2^16
            uint32_t w4[4];
            spread8(pc, w4);
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
    block_scan_256(part, [] { return (uint64_t) 0; }, [=](uint64_t total) { tot1[b] = total; });
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
    block_scan_256(part, [] { return (uint64_t) 0; }, [=](uint64_t total) { binstart1[bins1] = total; });
    uint64_t run = part[threadIdx.x];
    for (uint32_t b = b0; b < b1; b++) { binstart1[b] = run; run += tot1[b]; }
}

// level 1, pass 2 of the exact route (private ranges per unit from the histogram), and the owner grouping of a distributed add
__global__ void __launch_bounds__(SCATTER_THREADS) k_part_scatter1_exact(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, PartPlan pl,
                                                                         const uint64_t *offs1, const uint64_t *binstart1, uint64_t *out) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t bins1 = plan_bins1(pl);
    ScatterLds l = scatter_lds(smem, bins1);
    scatter_open(l, bins1, [&](uint32_t b) { return binstart1[b] + offs1[(uint64_t) blockIdx.x * bins1 + b]; });
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const UnitSteps u = unit_steps(0, pl.steps_per_unit, flat_wave_steps(total));
    uint32_t r_hint = 0xFFFFFFFFu, w0, ex;
    const Digit d1 = plan_digit1(pl);
    for (uint64_t t0 = u.s0; t0 < u.s1; t0 += u.nwaves) {
        uint64_t it[16];
        flat_step_load(bases, total, t0 + u.wave, t0 + u.wave < u.s1, w0, ex);
        flat_step_items(offsets, n_seq, total, start, k, t0 + u.wave, t0 + u.wave < u.s1, w0, ex, r_hint, it);
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
__global__ void __launch_bounds__(SCATTER_THREADS) k_part_scatter1(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, PartPlan pl,
                                                                   uint64_t *out, SegPlan1 seg) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    const uint32_t bins1 = plan_bins1(pl);
    SegLds ls = seg_lds(smem, bins1);
    SegOut sg;
    uint32_t *cursor;
    seg_open(ls, bins1, blockIdx.x % seg.sets, seg.cap, seg.ovf, seg.state, sg, cursor);
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t nsteps_all = flat_wave_steps(total);
    const uint64_t nsteps = seg.step_end ? seg.step_end : nsteps_all;
    const UnitSteps u = unit_steps(seg.step_base, pl.steps_per_unit, nsteps);
    uint32_t w0, ex, bad = 0;
    FlatRaw raw;
    const uint64_t last_step = nsteps_all ? nsteps_all - 1 : 0;
    flat_step_fetch(bases, total, u.s0 + u.wave, raw, seg.novalid, last_step);
    vm_wait_all();
    const Digit d1 = plan_digit1(pl);
    for (uint64_t t0 = u.s0; t0 < u.s1; t0 += u.nwaves) {
        uint64_t it[16];
        flat_step_words(bases, total, start, t0 + u.wave, t0 + u.wave < u.s1, raw, w0, ex, bad);
        flat_step_items_nv(k, t0 + u.wave < u.s1, w0, ex, raw.nv, it);
        // the next step's chunks and its "no k-mer" bits are requested now; they arrive under the tile sort, which waits for them
        // before its write-out
        flat_step_fetch(bases, total, t0 + u.nwaves + u.wave, raw, seg.novalid, last_step);
#pragma unroll
        for (int j = 0; j < 16; j++) it[j] = khash(it[j]); // from here on the k-mers travel as their table hash (khash keeps the "no k-mer" mark)
        tile_scatter_seg<true, false, false, 0>(it, ls, bins1, d1, out, sg, cursor);
    }
    if (bad) atomicOr(seg.err, DERR_NON_ACGT);
}

} // namespace kmu

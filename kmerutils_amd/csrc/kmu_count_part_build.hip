// kmu_count_part_build.hip -- the last stage of the partitioned build: one workgroup per region builds the region in LDS (ds_cmpst / ds_add)
// from its leaf and streams its image out; the spill list follows by direct insertion (host side: kmu_count_part.hip; declarations and
// constants: kmu_count_part_kernels.h; the 6-byte leaf item that level 2 writes: kmu_count_part_steps.h).
#include "kmu_count_part_steps.h"

namespace kmu {

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

// the spill list of a single-pass partition (khash values) into the finished table, by direct insertion
__global__ void __launch_bounds__(256) k_count_add_spill(const uint64_t *items, const uint32_t *ovf, CountTable t, uint32_t *err) {
    const uint32_t n = ovf[1] < ovf[2] ? ovf[1] : ovf[2];
    bool full = false;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        if (!count_insert_h(t, t.w ? 0ull : khash_inv(items[i]), items[i], 1u)) full = true;
    if (full) atomicOr(err, DERR_TABLE_FULL);
}

// the forms the host side launches (kmu_count_part_kernels.h)
#define KMU_X_INST(...) template __global__ void __VA_ARGS__;
KMU_COUNT_PART_BUILD_FORMS(KMU_X_INST)
#undef KMU_X_INST

} // namespace kmu

// kmu_sketch_groups.hip -- kmu_sketch_groups: one signature per GROUP of consecutive sequences in one call; row g is what
// kmu_sketch(KMU_MODE_ALL_SEQS) gives for the sequences of group g alone.  Reference: SeqSketcherT::sketch_compressedkmer_seqs
// called once per genome / proteome file (src/sketching/setsketchert.rs:160-202, 299-335, 1007-1045).
//
// Routes (the kernel launches and host synchronisations of a call do not depend on the number of groups):
//  ProbMinHash3a / 3   k_nk_scan + k_seq_hashes_compact over all sequences (groups are runs of consecutive sequences, so the
//                      compact hash array is already grouped), k_group_plan, a segmented partition of every group into leaves
//                      of ~4 k keys (k_grp_hist, k_grp_bounds, k_grp_scatter), ONE k_sketch_pmh3a over the leaves of all
//                      groups, k_pmh_reduce_groups.
//                      Exact because a key's weight is its multiplicity over its group and the signature is the per-slot
//                      minimum of (h, key) over disjoint key sets: equal keys of one group land in one leaf (the leaf is a
//                      function of (group, key)); nothing else about the cut, nor the order inside a leaf, matters.
//  SuperMinHash(2)     items are independent: chunks of <= 16 384 hashes that never straddle a group (k_grp_chunk_offsets),
//                      ONE k_sketch_super over all chunks, k_super_reduce_groups.
//  OptDens / RevOptDens / HLL   no hashes, no plan the host sees: k_grp_dens_plan checks group_offsets, flags empty sequences, fills
//                      one row of bins / registers per group and cuts the concatenated bases into tiles of equally many bases;
//                      ONE persistent k_grp_dens_walk takes tiles from a queue, finds the sequences and groups of a tile by binary
//                      search, walks their steps straight from the bases (oph_walk) into bins in LDS and merges them into the
//                      group's row whenever the group changes; k_grp_dens_finish densifies and stores row g.
//                      Exact because a bin is a minimum and a register a maximum over independent k-mer occurrences: every step
//                      of every sequence is walked by exactly one wave (the tile its first base lies in), and no cut or order
//                      of minima / maxima changes them.
#include <algorithm>
#include <vector>

#include "kmu_sketch_dens.h"
#include "kmu_sketch_host.hpp"
#include "kmu_sketch_kernels.h"

namespace kmu {

static constexpr uint64_t GRP_H_INIT = 0x7FEFFFFFFFFFFFFFull; // an empty slot of k_sketch_pmh3a's partial rows: bits of f64::MAX
static constexpr uint32_t GRP_TILE = 4096;                    // keys a workgroup takes at a time: 16 per thread
static constexpr uint32_t GRP_LDS_BITS = 12;                  // groups of up to 2^12 leaves count their tiles in LDS
static constexpr uint32_t GRP_BAD_START = 1u, GRP_BAD_ORDER = 2u, GRP_BAD_END = 4u;

// the groups on the device: group g holds the hashes [gk[g], gk[g + 1]) and the leaves (chunks) [leaf_base[g], leaf_base[g + 1])
struct GroupArgs {
    const uint64_t *gk;        // n_groups + 1
    const uint64_t *leaf_base; // n_groups + 1
    const uint32_t *bits;      // ProbMinHash: group g has 2^bits[g] leaves
    uint32_t n_groups;
};

// leaf of a key inside its group (b >= 1): the top bits of a 64-bit finaliser (MurmurHash3's)
__device__ __forceinline__ uint32_t grp_bucket(uint64_t x, uint32_t b) {
    x ^= x >> 33;
    x *= 0xff51afd7ed558ccdull;
    x ^= x >> 33;
    x *= 0xc4ceb9fe1a85ec53ull;
    x ^= x >> 33;
    return (uint32_t) (x >> (64 - b));
}
// the group of item i, searched in [lo, hi] (gk[lo] <= i < gk[hi + 1]): the last g with gk[g] <= i -- never an empty group
// (k_grp_dens_walk: also the sequence of a base in `offsets`, never an empty sequence)
__device__ __forceinline__ uint32_t grp_of(const uint64_t *gk, uint32_t lo, uint32_t hi, uint64_t i) {
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo + 1) / 2;
        if (gk[mid] <= i) lo = mid;
        else hi = mid - 1;
    }
    return lo;
}
__device__ __forceinline__ uint64_t grp_shfl_up(uint64_t v, int d) {
    return ((uint64_t) (uint32_t) __shfl_up((int) (v >> 32), d, 64) << 32) | (uint32_t) __shfl_up((int) (uint32_t) v, d, 64);
}
// exclusive scan of v over a workgroup of 1024 threads, on top of *carry; *carry becomes the running total.  All threads call it.
__device__ __forceinline__ uint64_t grp_block_scan(uint64_t v, uint64_t *wtot, uint64_t *carry) {
    uint64_t incl = v;
    for (int d = 1; d < 64; d <<= 1) {
        const uint64_t o = grp_shfl_up(incl, d);
        if (lane_id() >= d) incl += o;
    }
    if (lane_id() == 63) wtot[threadIdx.x >> 6] = incl;
    __syncthreads();
    uint64_t pre = *carry;
    for (int w = 0; w < (int) (threadIdx.x >> 6); w++) pre += wtot[w];
    __syncthreads();
    if (threadIdx.x == blockDim.x - 1) *carry = pre + incl;
    __syncthreads();
    return pre + incl - v;
}

// The plan of a call, one workgroup: checks group_offsets (every index is clamped to n_seq before it is used, so a malformed
// array is never read through), gk[g] = koff[group_offsets[g]], the leaves (super: chunks) of every group and their exclusive
// scan.  head: [0] hashes of the call, [1] leaves of the call, [2] GRP_BAD_* bits.
__global__ void __launch_bounds__(1024) k_group_plan(const uint64_t *go, uint32_t n_groups, uint32_t n_seq, const uint64_t *koff, int super,
                                                     uint64_t *gk, uint64_t *leaf_base, uint32_t *bits, uint64_t *head) {
    __shared__ uint64_t wtot[16];
    __shared__ uint64_t carry;
    __shared__ uint32_t bad;
    if (threadIdx.x == 0) {
        carry = 0;
        bad = 0;
    }
    __syncthreads();
    for (uint32_t base = 0; base < n_groups; base += blockDim.x) {
        const uint32_t g = base + threadIdx.x;
        uint64_t v = 0;
        if (g < n_groups) {
            const uint64_t s0 = go[g], s1 = go[g + 1];
            uint32_t e = 0;
            if (g == 0 && s0 != 0) e |= GRP_BAD_START;
            if (s1 < s0) e |= GRP_BAD_ORDER;
            if (g == n_groups - 1 && s1 != (uint64_t) n_seq) e |= GRP_BAD_END;
            if (e) atomicOr(&bad, e);
            const uint64_t k0 = koff[s0 < n_seq ? s0 : n_seq], k1 = koff[s1 < n_seq ? s1 : n_seq];
            const uint64_t n = k1 > k0 ? k1 - k0 : 0;
            gk[g] = k0;
            if (g == n_groups - 1) gk[n_groups] = k1;
            if (super) v = super_chunk_count(n);
            else {
                const uint32_t b = pmh_leaf_bits(n);
                bits[g] = b;
                v = 1ull << b;
            }
        }
        const uint64_t excl = grp_block_scan(v, wtot, &carry);
        if (g < n_groups) leaf_base[g] = excl;
    }
    if (threadIdx.x == 0) {
        leaf_base[n_groups] = carry;
        head[0] = koff[n_seq];
        head[1] = carry;
        head[2] = bad;
    }
}

// keys per leaf.  A tile inside one group counts in LDS and adds its non-empty bins at the end; a tile across a group
// boundary (and a group of more than 2^12 leaves) counts key by key.  Single-leaf groups are not counted: k_grp_bounds knows them.
__global__ void __launch_bounds__(256) k_grp_hist(const uint64_t *keys, uint64_t n, GroupArgs ga, unsigned long long *cnt) {
    __shared__ uint32_t h[1u << GRP_LDS_BITS];
    __shared__ uint32_t sg[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = (n + GRP_TILE - 1) / GRP_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * GRP_TILE, t1 = t0 + GRP_TILE < n ? t0 + GRP_TILE : n;
        if (tid == 0) {
            sg[0] = grp_of(ga.gk, 0, ga.n_groups - 1, t0);
            sg[1] = grp_of(ga.gk, sg[0], ga.n_groups - 1, t1 - 1);
        }
        __syncthreads();
        const uint32_t g0 = sg[0], g1 = sg[1];
        __syncthreads();
        if (g0 == g1) {
            const uint32_t b = ga.bits[g0];
            if (b == 0) continue;
            const uint64_t lb = ga.leaf_base[g0];
            if (b <= GRP_LDS_BITS) {
                for (uint32_t x = tid; x < (1u << b); x += 256) h[x] = 0;
                __syncthreads();
                for (uint32_t j = 0; j < GRP_TILE / 512; j++) {
                    const uint64_t i = t0 + ((uint64_t) j * 256 + tid) * 2;
                    if (i + 1 < t1) {
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(keys + i);
                        atomicAdd(&h[grp_bucket(v.x, b)], 1u);
                        atomicAdd(&h[grp_bucket(v.y, b)], 1u);
                    } else if (i < t1)
                        atomicAdd(&h[grp_bucket(keys[i], b)], 1u);
                }
                __syncthreads();
                for (uint32_t x = tid; x < (1u << b); x += 256)
                    if (h[x]) atomicAdd(&cnt[lb + x], (unsigned long long) h[x]);
                __syncthreads();
            } else {
                for (uint64_t i = t0 + tid; i < t1; i += 256) atomicAdd(&cnt[lb + grp_bucket(keys[i], b)], 1ull);
            }
        } else {
            for (uint64_t i = t0 + tid; i < t1; i += 256) {
                const uint32_t g = grp_of(ga.gk, g0, g1, i), b = ga.bits[g];
                if (b) atomicAdd(&cnt[ga.leaf_base[g] + grp_bucket(keys[i], b)], 1ull);
            }
        }
    }
}

// the leaves' bounds in the partitioned array: inside group g an exclusive scan of its counts on top of gk[g].  One workgroup
// per group.  cnt holds the counts on entry and the same bounds on exit: the cursors of k_grp_scatter.
__global__ void __launch_bounds__(1024) k_grp_bounds(GroupArgs ga, unsigned long long *cnt, uint64_t *bounds) {
    __shared__ uint64_t wtot[16];
    __shared__ uint64_t carry;
    for (uint32_t g = blockIdx.x; g < ga.n_groups; g += gridDim.x) {
        const uint32_t b = ga.bits[g];
        const uint64_t lb = ga.leaf_base[g], first = ga.gk[g];
        if (b == 0) {
            if (threadIdx.x == 0) {
                bounds[lb] = first;
                cnt[lb] = first;
            }
        } else {
            __syncthreads();
            if (threadIdx.x == 0) carry = first;
            __syncthreads();
            const uint64_t nb = 1ull << b;
            for (uint64_t x0 = 0; x0 < nb; x0 += blockDim.x) {
                const uint64_t x = x0 + threadIdx.x;
                const uint64_t v = x < nb ? (uint64_t) cnt[lb + x] : 0;
                const uint64_t excl = grp_block_scan(v, wtot, &carry);
                if (x < nb) {
                    bounds[lb + x] = excl;
                    cnt[lb + x] = excl;
                }
            }
        }
        if (g == ga.n_groups - 1 && threadIdx.x == 0) bounds[ga.leaf_base[ga.n_groups]] = ga.gk[ga.n_groups];
    }
}

// the keys into their leaves.  A tile inside one group ranks its keys per leaf in LDS and reserves one range per non-empty leaf
// with one atomic; a key of a single-leaf group keeps its place (a copy).  The order inside a leaf is arbitrary: a leaf is a multiset.
__global__ void __launch_bounds__(256) k_grp_scatter(const uint64_t *keys, uint64_t n, GroupArgs ga, unsigned long long *cursor,
                                                     uint64_t *out) {
    __shared__ uint32_t h[1u << GRP_LDS_BITS];
    __shared__ uint32_t sg[2];
    const uint32_t tid = threadIdx.x;
    const uint64_t n_tiles = (n + GRP_TILE - 1) / GRP_TILE;
    for (uint64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const uint64_t t0 = tile * GRP_TILE, t1 = t0 + GRP_TILE < n ? t0 + GRP_TILE : n;
        if (tid == 0) {
            sg[0] = grp_of(ga.gk, 0, ga.n_groups - 1, t0);
            sg[1] = grp_of(ga.gk, sg[0], ga.n_groups - 1, t1 - 1);
        }
        __syncthreads();
        const uint32_t g0 = sg[0], g1 = sg[1];
        __syncthreads();
        if (g0 == g1) {
            const uint32_t b = ga.bits[g0];
            const uint64_t lb = ga.leaf_base[g0], first = ga.gk[g0];
            if (b == 0) {
                for (uint32_t j = 0; j < GRP_TILE / 512; j++) {
                    const uint64_t i = t0 + ((uint64_t) j * 256 + tid) * 2;
                    if (i + 1 < t1) *reinterpret_cast<ulonglong2 *>(out + i) = *reinterpret_cast<const ulonglong2 *>(keys + i);
                    else if (i < t1) out[i] = keys[i];
                }
            } else if (b <= GRP_LDS_BITS) {
                constexpr uint32_t NONE = 0xFFFFFFFFu;
                uint64_t k[GRP_TILE / 256];
                uint32_t rk[GRP_TILE / 256];
                for (uint32_t x = tid; x < (1u << b); x += 256) h[x] = 0;
                __syncthreads();
#pragma unroll
                for (uint32_t j = 0; j < GRP_TILE / 512; j++) {
                    const uint64_t i = t0 + ((uint64_t) j * 256 + tid) * 2;
                    k[2 * j] = k[2 * j + 1] = 0;
                    rk[2 * j] = rk[2 * j + 1] = NONE;
                    if (i + 1 < t1) {
                        const ulonglong2 v = *reinterpret_cast<const ulonglong2 *>(keys + i);
                        k[2 * j] = v.x;
                        k[2 * j + 1] = v.y;
                        rk[2 * j] = atomicAdd(&h[grp_bucket(v.x, b)], 1u);
                        rk[2 * j + 1] = atomicAdd(&h[grp_bucket(v.y, b)], 1u);
                    } else if (i < t1) {
                        k[2 * j] = keys[i];
                        rk[2 * j] = atomicAdd(&h[grp_bucket(k[2 * j], b)], 1u);
                    }
                }
                __syncthreads();
                // (a group of at most 2^12 leaves has fewer than 2^25 keys: places relative to the group's first fit 32 bits)
                for (uint32_t x = tid; x < (1u << b); x += 256) {
                    const uint32_t c = h[x];
                    if (c) h[x] = (uint32_t) ((uint64_t) atomicAdd(&cursor[lb + x], (unsigned long long) c) - first);
                }
                __syncthreads();
#pragma unroll
                for (uint32_t j = 0; j < GRP_TILE / 256; j++)
                    if (rk[j] != NONE) out[first + h[grp_bucket(k[j], b)] + rk[j]] = k[j];
                __syncthreads();
            } else {
                for (uint64_t i = t0 + tid; i < t1; i += 256) {
                    const uint64_t key = keys[i];
                    out[atomicAdd(&cursor[lb + grp_bucket(key, b)], 1ull)] = key;
                }
            }
        } else {
            for (uint64_t i = t0 + tid; i < t1; i += 256) {
                const uint32_t g = grp_of(ga.gk, g0, g1, i), b = ga.bits[g];
                const uint64_t key = keys[i];
                if (b == 0) out[i] = key;
                else out[atomicAdd(&cursor[ga.leaf_base[g] + grp_bucket(key, b)], 1ull)] = key;
            }
        }
    }
}

// k_pmh_reduce per group: per slot the smallest (h, key) over the leaves of group blockIdx.x.  A wave reads 64 consecutive slots
// of one leaf row (512 contiguous bytes), the four waves of the workgroup take every fourth leaf.
__global__ void __launch_bounds__(256) k_pmh_reduce_groups(const uint64_t *part_h, const uint64_t *part_k, const uint64_t *leaf_base, int m,
                                                           int sig_bytes, void *sig_out) {
    __shared__ uint64_t sh[256], sk[256];
    const uint32_t g = blockIdx.x, lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    const uint64_t l0 = leaf_base[g], l1 = leaf_base[g + 1];
    for (uint32_t st = blockIdx.y; st * 64u < (uint32_t) m; st += gridDim.y) {
        const uint32_t t = st * 64u + lane;
        uint64_t bh = GRP_H_INIT, bk = 0;
        if (t < (uint32_t) m)
            for (uint64_t i = l0 + w; i < l1; i += 4) {
                const uint64_t hh = part_h[i * (uint64_t) m + t], key = part_k[i * (uint64_t) m + t];
                if (hh < bh || (hh == bh && hh != GRP_H_INIT && key < bk)) { bh = hh; bk = key; }
            }
        sh[threadIdx.x] = bh;
        sk[threadIdx.x] = bk;
        __syncthreads();
        if (w == 0 && t < (uint32_t) m) {
            for (uint32_t ww = 1; ww < 4; ww++) {
                const uint64_t hh = sh[ww * 64 + lane], key = sk[ww * 64 + lane];
                if (hh < bh || (hh == bh && hh != GRP_H_INIT && key < bk)) { bh = hh; bk = key; }
            }
            const uint64_t v = bh == GRP_H_INIT ? 0ull : bk;
            if (sig_bytes == 4) reinterpret_cast<uint32_t *>(sig_out)[(uint64_t) g * m + t] = (uint32_t) v;
            else reinterpret_cast<uint64_t *>(sig_out)[(uint64_t) g * m + t] = v;
        }
        __syncthreads();
    }
}

// the chunks of every group: chunk c of nc starts at gk[g] + n c / nc (one wave per group)
__global__ void __launch_bounds__(256) k_grp_chunk_offsets(GroupArgs ga, uint64_t *off) {
    const uint32_t wave = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), n_waves = gridDim.x * (blockDim.x >> 6);
    for (uint32_t g = wave; g < ga.n_groups; g += n_waves) {
        const uint64_t k0 = ga.gk[g], n = ga.gk[g + 1] - k0, lb = ga.leaf_base[g], nc = ga.leaf_base[g + 1] - lb;
        for (uint64_t c = lane_id(); c < nc; c += 64) off[lb + c] = k0 + n * c / nc;
        if (g == ga.n_groups - 1 && lane_id() == 0) off[lb + nc] = k0 + n;
    }
}

// k_super_reduce per group: element-wise minimum of the chunk rows of group blockIdx.x (order-preserving bit patterns)
__global__ void __launch_bounds__(256) k_super_reduce_groups(const uint64_t *part_rows, const uint64_t *leaf_base, int m, int mode,
                                                             uint64_t init_bits, void *sig_out) {
    const uint32_t g = blockIdx.x;
    const uint64_t l0 = leaf_base[g], l1 = leaf_base[g + 1];
    for (uint32_t t = blockIdx.y * blockDim.x + threadIdx.x; t < (uint32_t) m; t += gridDim.y * blockDim.x) {
        uint64_t best = init_bits;
        for (uint64_t i = l0; i < l1; i++) {
            const uint64_t v = part_rows[i * (uint64_t) m + t];
            best = v < best ? v : best;
        }
        if (mode == 0 || mode == 2) reinterpret_cast<uint64_t *>(sig_out)[(uint64_t) g * m + t] = best;
        else reinterpret_cast<uint32_t *>(sig_out)[(uint64_t) g * m + t] = (uint32_t) best;
    }
}

// ---- OptDens / RevOptDens / HLL ----------------------------------------------------------------------------------------------
// head of the route (u64 words): first base, end of the bases, bases per tile, GRP_BAD_* bits
enum { GD_BASE0 = 0, GD_END = 1, GD_TILE = 2, GD_BAD = 3, GD_WORDS = 4 };
static constexpr uint64_t GD_TILE_MIN = 4096, GD_TILE_MAX = 1u << 17; // bases of a tile: one step per wave .. 32 per wave
static constexpr uint32_t GD_NONE = 0xFFFFFFFFu;
#ifndef KMU_GRP_HLL_SEED
#define KMU_GRP_HLL_SEED 1 // (0: diagnostics, scripts/build_variant.sh -- every unit starts its K_low at 0)
#endif

// Before the walk, the whole grid: group_offsets checked (as k_group_plan checks them; nothing is read through them here), an empty
// sequence is KMU_E_EMPTY_SEQ wherever it stands, the n_groups rows start neutral, and the tile: as many bases as give every
// workgroup of the walk ~4 turns, a multiple of the DNA step, within [GD_TILE_MIN, GD_TILE_MAX].
__global__ void __launch_bounds__(256) k_grp_dens_plan(const uint64_t *go, uint32_t n_groups, const uint64_t *offsets, uint32_t n_seq,
                                                       uint64_t *rows, uint64_t n_rows_words, uint64_t neutral, uint32_t walk_grid,
                                                       unsigned long long *head, uint32_t *err) {
    const uint64_t tid = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x, nthreads = (uint64_t) gridDim.x * blockDim.x;
    uint32_t e = 0;
    for (uint64_t g = tid; g < n_groups; g += nthreads) {
        const uint64_t s0 = go[g], s1 = go[g + 1];
        if (g == 0 && s0 != 0) e |= GRP_BAD_START;
        if (s1 < s0) e |= GRP_BAD_ORDER;
        if (g == n_groups - 1 && s1 != (uint64_t) n_seq) e |= GRP_BAD_END;
    }
    if (e) atomicOr(&head[GD_BAD], (unsigned long long) e);
    bool empty = false;
    for (uint64_t i = tid; i < n_seq; i += nthreads) empty |= offsets[i + 1] == offsets[i];
    if (empty) atomicOr(err, DERR_EMPTY_SEQ);
    for (uint64_t i = tid; i < n_rows_words; i += nthreads) rows[i] = neutral;
    if (tid == 0) {
        const uint64_t b0 = offsets[0], b1 = offsets[n_seq], total = b1 > b0 ? b1 - b0 : 0, turns = (uint64_t) walk_grid * 4;
        uint64_t tile = ((total + turns - 1) / turns + 1023) / 1024 * 1024;
        tile = tile < GD_TILE_MIN ? GD_TILE_MIN : tile > GD_TILE_MAX ? GD_TILE_MAX : tile;
        head[GD_BASE0] = b0;
        head[GD_END] = b0 + total;
        head[GD_TILE] = tile;
    }
}

// The bins / registers of all groups.  Persistent workgroups take tiles [t0, t1) of the concatenated bases from a queue.  Step st
// of sequence r (oph_steps: 1024 bases from base 1024 st - lead, 64 residues from residue 64 st) belongs to the tile that holds
// its first base offsets[r] + max(0, 1024 st - lead) -- every step to exactly one tile, whatever the sequences' lengths: work is
// cut by amount of sequence.  The four waves share the steps of a tile round-robin across sequence boundaries (`c`), so a tile of
// many short reads keeps them all busy; they only meet where the group changes.  The bins stay in LDS across tiles while the
// group is the same and are merged into the group's row (oph_merge_to_row) when it changes and at the end.
// LDS: hs[m] | w[8]: w[0] this tile, w[1] K_low, w[4 .. 7] the waves' minima of the group's row.
template <bool HLL>
__global__ void __launch_bounds__(256) k_grp_dens_walk(DensArgs a, const uint64_t *go, uint32_t n_groups, uint64_t *rows,
                                                       const unsigned long long *head) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *hs = reinterpret_cast<uint64_t *>(smem);
    uint32_t *w = reinterpret_cast<uint32_t *>(hs + a.m);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const uint32_t wave = (uint32_t) tid >> 6;
    const bool aa = a.cfg.kmer_type == KMU_KMERAA32BIT || a.cfg.kmer_type == KMU_KMERAA64BIT;
    const uint64_t step_len = aa ? 64 : 1024;
    const uint64_t neutral = oph_neutral(a);
    const uint64_t base0 = head[GD_BASE0], end = head[GD_END], tile = head[GD_TILE];
    const uint64_t n_tiles = (end - base0 + tile - 1) / tile;
    const uint32_t n_seq = a.n_seq;
    uint32_t cur_g = GD_NONE, bad = 0;
    if (tid == 0) w[0] = atomicAdd(a.queue, 1u);
    __syncthreads();
    for (;;) {
        const uint64_t t = w[0];
        __syncthreads(); // everyone holds t before thread 0 posts the next one
        if (t >= n_tiles) break;
        uint32_t t_next = 0;
        if (tid == 0) t_next = atomicAdd(a.queue, 1u);
        const uint64_t t0 = base0 + t * tile, t1 = t0 + tile < end ? t0 + tile : end;
        const uint32_t r0 = grp_of(a.offsets, 0, n_seq - 1, t0), r1 = grp_of(a.offsets, r0, n_seq - 1, t1 - 1);
        uint32_t c = 0; // steps of this tile so far, modulo the waves
        for (uint32_t r = r0; r <= r1;) {
            const uint32_t g = grp_of(go, cur_g != GD_NONE ? cur_g : 0, n_groups - 1, (uint64_t) r) /* (tiles and sequences only go up) */;
            const uint64_t g_end = go[g + 1] < (uint64_t) n_seq ? go[g + 1] : (uint64_t) n_seq; // (clamped like every index taken from go)
            uint32_t r_end = g_end - 1 < (uint64_t) r1 ? (uint32_t) (g_end - 1) : r1;
            r_end = r_end < r ? r : r_end;
            if (g != cur_g) {
                __syncthreads(); // the waves are through with the group before
                if (cur_g != GD_NONE) {
                    a.row = rows + (uint64_t) cur_g * a.m;
                    oph_merge_to_row(a, hs);
                }
                for (int s = tid; s < a.m; s += nthreads) hs[s] = neutral; // (the entries this thread merged)
                if constexpr (HLL) {
                    // K_low of the new group: never the one of the group before.  Seeded with the minimum of the group's global
                    // row as it stands -- exact: the global registers only grow, so their minimum now is a lower bound of the
                    // final registers, and an update with k <= that bound changes none of them.  Only where other units may
                    // have merged into the row: a group that reaches beyond this tile.
                    uint64_t mn = 0;
                    const uint64_t g_first = go[g] < (uint64_t) n_seq ? go[g] : (uint64_t) n_seq;
                    if (KMU_GRP_HLL_SEED && (a.offsets[g_first] < t0 || a.offsets[g_end] > t1)) {
                        mn = ~0ull;
                        for (int s = tid; s < a.m; s += nthreads) {
                            const uint64_t v = __hip_atomic_load(&rows[(uint64_t) g * a.m + s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                            mn = v < mn ? v : mn;
                        }
                        mn = ~wave_max_u64(~mn);
                    }
                    if (lane_id() == 0) w[4 + wave] = (uint32_t) mn;
                    __syncthreads();
                    if (tid == 0) w[1] = min(min(w[4], w[5]), min(w[6], w[7]));
                }
                __syncthreads();
                cur_g = g;
            }
            for (uint32_t rr = r; rr <= r_end; rr++) {
                const SeqView sv = dens_view(a, rr);
                if (sv.len == 0) continue; // (KMU_E_EMPTY_SEQ: k_grp_dens_plan)
                const uint64_t off = a.offsets[rr], lead = aa ? 0 : seq_lead(sv), n_st = oph_steps(sv, aa);
                const uint64_t lo = t0 > off ? (t0 - off + lead + step_len - 1) / step_len : 0;
                uint64_t hi = (t1 - off + lead + step_len - 1) / step_len;
                hi = hi < n_st ? hi : n_st;
                if (lo >= hi) continue;
                const uint64_t nk = sv.len >= (uint64_t) a.cfg.k ? sv.len - a.cfg.k + 1 : 0; // 0: the walk only validates
                bad |= oph_walk<HLL>(a, sv, hs, &w[1], aa, nk, lo + ((wave - c) & 3u), 4, hi);
                c += (uint32_t) (hi - lo);
            }
            r = r_end + 1;
        }
        if (tid == 0) w[0] = t_next;
        __syncthreads();
    }
    if (cur_g != GD_NONE) { // (the break above came after a barrier behind the last walk)
        a.row = rows + (uint64_t) cur_g * a.m;
        oph_merge_to_row(a, hs);
    }
    if (bad) atomicOr(a.err, aa ? DERR_BAD_AA : DERR_NON_ACGT);
}

// k_oph_finish per group: the group's row -> LDS -> densified (not HLL) -> signature row g
__global__ void __launch_bounds__(256) k_grp_dens_finish(DensArgs a, const uint64_t *rows, uint32_t n_groups) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *hs;
    uint32_t *filled, *cnt, *claim;
    oph_lds(a, smem, hs, filled, cnt, claim);
    for (uint32_t g = blockIdx.x; g < n_groups; g += gridDim.x) {
        for (int s = threadIdx.x; s < a.m; s += blockDim.x) {
            hs[s] = rows[(uint64_t) g * a.m + s];
            if (a.rev) claim[s] = 0xFFFFFFFFu;
        }
        __syncthreads();
        if (!a.hll) oph_densify(a, hs, filled, claim, cnt);
        oph_store_row(a, hs, (uint64_t) g);
        __syncthreads();
    }
}

} // namespace kmu

using namespace kmu;

static const char *groups_bad_text(uint32_t bits) {
    return bits & GRP_BAD_START ? "group_offsets[0] must be 0"
           : bits & GRP_BAD_ORDER ? "group_offsets must not decrease"
                                  : "group_offsets[n_groups] must be n_seq";
}
static uint32_t groups_check_host(const uint64_t *go, uint32_t n_groups, uint32_t n_seq) {
    uint32_t e = go[0] != 0 ? GRP_BAD_START : 0u;
    for (uint32_t g = 0; g < n_groups; g++)
        if (go[g + 1] < go[g]) e |= GRP_BAD_ORDER;
    if (go[n_groups] != (uint64_t) n_seq) e |= GRP_BAD_END;
    return e;
}

// OptDens / RevOptDens / HLL: plan, one walk over all groups, finish.  host_checked: group_offsets were checked on the host
// (host memory); else their check bits are the one device-to-host copy of the call.
static int groups_dens(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_go, uint32_t n_groups, void *d_sig,
                       uint32_t *d_err, bool host_checked) {
    DensArgs a;
    dens_args(ctx, p, ds, d_sig, d_err, nullptr, 0, &a);
    const void *fns[3] = {(const void *) k_grp_dens_walk<false>, (const void *) k_grp_dens_walk<true>, (const void *) k_grp_dens_finish};
    KMU_TRY(dens_lds_check(ctx, a, fns, 3));
    const size_t lds_full = dens_lds_full(a), lds_walk = (size_t) 8 * a.m + 32;
    const uint64_t n_words = (uint64_t) n_groups * a.m;
    uint64_t *rows;
    void *head, *q;
    KMU_TRY(dev_array(ctx, "grp.rows", n_words + 8, &rows));
    KMU_TRY(dev_buf(ctx, "grp.head", 64, &head));
    KMU_TRY(dev_buf(ctx, "queue", 64, &q));
    KMU_HIP(ctx, hipMemsetAsync(head, 0, 64, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(q, 0, 64, ctx->stream));
    a.queue = (uint32_t *) q;
    // persistent: the workgroups a CU holds, by LDS and by registers (82 VGPRs: five waves per SIMD; the HLL walk 150: three)
    const unsigned walk_grid = (unsigned) ctx->num_cus * (unsigned) std::max<size_t>(1, std::min<size_t>(a.hll ? 3 : 5, DENS_LDS_MAX / lds_walk));
    const uint64_t work = std::max<uint64_t>(std::max<uint64_t>(n_words, ds.n_seq), n_groups);
    KMU_TRY(launch(ctx, "k_grp_dens_plan", k_grp_dens_plan, dim3((unsigned) std::min<uint64_t>((work + 255) / 256, (uint64_t) ctx->num_cus * 8)),
                   dim3(256), 0, d_go, n_groups, ds.offsets, ds.n_seq, rows, n_words, dens_neutral_bits(a), walk_grid, (unsigned long long *) head,
                   d_err));
    if (!host_checked) {
        uint64_t h_head[GD_WORDS] = {0, 0, 0, 0}; // the one device-to-host copy of the call
        KMU_TRY(read_back(ctx, {{h_head, head, sizeof h_head}}));
        if (h_head[GD_BAD]) {
            if (!ctx->async_device) (void) check_err_word(ctx, d_err); // (read, so that it starts clear next time)
            return fail(ctx, KMU_E_BAD_ARG, "%s", groups_bad_text((uint32_t) h_head[GD_BAD]));
        }
    }
    KMU_TRY(launch(ctx, "k_grp_dens_walk", a.hll ? k_grp_dens_walk<true> : k_grp_dens_walk<false>, dim3(walk_grid), dim3(256), lds_walk, a, d_go,
                   n_groups, rows, (const unsigned long long *) head));
    const unsigned per_cu = (unsigned) std::max<size_t>(1, std::min<size_t>(8, DENS_LDS_MAX / lds_full));
    return launch(ctx, "k_grp_dens_finish", k_grp_dens_finish, dim3(std::min<uint32_t>(n_groups, (uint32_t) ctx->num_cus * per_cu)), dim3(256),
                  lds_full, a, rows, n_groups);
}

// ProbMinHash3a / 3 and SuperMinHash(2): one batched pass over all groups
static int groups_batched(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_go, uint32_t n_groups,
                          void *d_sig, uint32_t *d_err) {
    const uint32_t n_seq = ds.n_seq;
    const int m = p->sketch_size;
    const bool super = p->algo != KMU_ALGO_PROB3A;
    uint64_t *hk, *lbase, *gk;
    uint32_t *bits;
    void *head;
    const uint64_t *koff;
    KMU_TRY(dev_array(ctx, "grp.gk", (size_t) n_groups + 1, &gk));
    KMU_TRY(dev_array(ctx, "grp.leaf_base", (size_t) n_groups + 1, &lbase));
    KMU_TRY(dev_array(ctx, "grp.bits", (size_t) n_groups, &bits));
    KMU_TRY(dev_buf(ctx, "grp.head", 64, &head));
    KMU_TRY(launch_nk_scan(ctx, ds, p->kmer_size, d_err, &koff));
    KMU_TRY(launch(ctx, "k_group_plan", k_group_plan, dim3(1), dim3(1024), 0, d_go, n_groups, n_seq, koff, super ? 1 : 0, gk, lbase, bits,
                   (uint64_t *) head));
    uint64_t h_head[3] = {0, 0, 0}; // the one device-to-host copy of the call
    KMU_TRY(read_back(ctx, {{h_head, head, sizeof h_head}}));
    if (h_head[2]) {
        if (!(p->mem == KMU_MEM_DEVICE && ctx->async_device)) (void) check_err_word(ctx, d_err); // (read, so that it starts clear next time)
        return fail(ctx, KMU_E_BAD_ARG, "%s", groups_bad_text((uint32_t) h_head[2]));
    }
    const uint64_t n_items = h_head[0], n_leaves = h_head[1];
    if (n_leaves > 0x7FFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu leaves in one call", (unsigned long long) n_leaves);
    KMU_TRY(dev_array(ctx, "all.hashes", n_items + 8, &hk));
    KMU_TRY(launch_hashes_compact(ctx, ds, KmerCfg{p->kmer_type, p->kmer_size, p->fhash}, koff, hk, d_err));
    GroupArgs ga{gk, lbase, bits, n_groups};
    const unsigned tile_grid = grid_for(ctx, n_items, GRP_TILE);
    const unsigned slot_tiles = (unsigned) std::min<uint32_t>(65535u, ((uint32_t) m + 63u) / 64u);
    if (!super) {
        uint64_t *pk, *ph, *items, *bounds;
        unsigned long long *cnt;
        KMU_TRY(dev_array(ctx, "grp.cursor", n_leaves + 8, &cnt));
        KMU_TRY(dev_array(ctx, "grp.bounds", n_leaves + 1 + 8, &bounds));
        KMU_TRY(dev_array(ctx, "grp.items", n_items + 8, &items));
        KMU_TRY(dev_array(ctx, "all.part_h", n_leaves * m, &ph));
        KMU_TRY(dev_array(ctx, "all.part_k", n_leaves * m, &pk));
        KMU_HIP(ctx, hipMemsetAsync(cnt, 0, n_leaves * 8, ctx->stream));
        KMU_TRY(launch(ctx, "k_grp_hist", k_grp_hist, dim3(tile_grid), dim3(256), 0, hk, n_items, ga, cnt));
        KMU_TRY(launch(ctx, "k_grp_bounds", k_grp_bounds, dim3(std::min<uint32_t>(n_groups, (uint32_t) ctx->num_cus * 2)), dim3(1024), 0, ga, cnt,
                       bounds));
        KMU_TRY(launch(ctx, "k_grp_scatter", k_grp_scatter, dim3(tile_grid), dim3(256), 0, hk, n_items, ga, cnt, items));
        KMU_TRY(launch_pmh3a_leaves(ctx, p, items, bounds, (uint32_t) n_leaves, ph,
                                    pk, d_err));
        KMU_TRY(launch(ctx, "k_pmh_reduce_groups", k_pmh_reduce_groups, dim3(n_groups, slot_tiles), dim3(256), 0, ph, pk, lbase, m,
                       kmer_val_bytes(p->kmer_type), d_sig));
        return KMU_OK;
    }
    // SuperMinHash / SuperMinHash2
    uint64_t *pr, *d_off;
    KMU_TRY(dev_array(ctx, "all.chunk_off", n_leaves + 1, &d_off));
    KMU_TRY(dev_array(ctx, "all.part_rows", n_leaves * m, &pr));
    KMU_TRY(launch(ctx, nullptr, k_grp_chunk_offsets,
                   dim3(grid_for(ctx, n_groups, 4)), dim3(256), 0, ga, d_off));
    KMU_TRY(launch_super(ctx, p, hashed_seqs(hk, d_off, (uint32_t) n_leaves), nullptr, d_err, hk, 8, pr));
    const int mode = super_mode(p);
    KMU_TRY(launch(ctx, "k_super_reduce_groups", k_super_reduce_groups,
                   dim3(n_groups, (unsigned) std::min<uint32_t>(65535u, ((uint32_t) m + 255u) / 256u)), dim3(256), 0, pr, lbase, m, mode,
                   super_init_bits(mode), d_sig));
    return KMU_OK;
}

extern "C" int kmu_sketch_groups(kmu_ctx *ctx, const kmu_sketch_params *p_in, const uint8_t *bases, const uint64_t *offsets,
                                 const uint64_t *packed_offsets, uint32_t n_seq, const uint64_t *group_offsets, uint32_t n_groups,
                                 void *sig_out) {
    if (!ctx || !p_in || !sig_out || !group_offsets) return KMU_E_BAD_ARG;
    kmu_sketch_params p_all = *p_in, p_res; // the checks kmu_sketch makes of an ALL_SEQS call, in its order and with its texts
    p_all.mode = KMU_MODE_ALL_SEQS;
    KMU_TRY(sketch_params(ctx, &p_all, &p_res));
    const kmu_sketch_params *p = &p_res;
    KMU_TRY(check_mem(ctx, p->mem));
    if (!offsets || (!bases && n_seq)) return fail(ctx, KMU_E_BAD_ARG, "null sequence buffers");
    if (n_groups == 0) return KMU_OK;
    const bool host = p->mem == KMU_MEM_HOST;
    if (host) {
        const uint32_t e = groups_check_host(group_offsets, n_groups, n_seq);
        if (e) return fail(ctx, KMU_E_BAD_ARG, "%s", groups_bad_text(e));
    }
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, packed_offsets, n_seq, p->input_kind, p->mem, &ds));
    const size_t row_bytes = (size_t) p->sketch_size * sig_elem_bytes(p->sig_type);
    uint8_t *d_sig;
    const uint64_t *d_go;
    KMU_TRY(place_output(ctx, "out.sig", (uint8_t *) sig_out, (size_t) n_groups * row_bytes + 64, p->mem, &d_sig));
    KMU_TRY(stage_to_device(ctx, "grp.go", group_offsets, (size_t) n_groups + 1, p->mem, &d_go));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    if (algo_is_dens(p->algo)) KMU_TRY(groups_dens(ctx, p, ds, d_go, n_groups, d_sig, d_err, host));
    else KMU_TRY(groups_batched(ctx, p, ds, d_go, n_groups, d_sig, d_err));
    KMU_TRY(bring_output(ctx, (uint8_t *) sig_out, d_sig, (size_t) n_groups * row_bytes, p->mem));
    return finish_checked(ctx, p->mem, d_err);
}

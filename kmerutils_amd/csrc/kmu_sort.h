// kmu_sort.h -- device sort of (u64 key, u32 value) entries: a stable LSD radix sort, 8-bit digits, up to eight passes.
//
// Per pass and per tile of SORT_TILE consecutive entries (one wave, a 64-thread workgroup, per tile):
//   k_sort_hist     the tile's count of every digit, hist[digit * n_tiles + tile]
//   device_scan_u32 an exclusive scan over that digit-major array: where the tile's entries of a digit go
//   k_sort_scatter  the tile again, 64 entries at a time in input order.  The lanes that hold the same digit find each other with
//                   eight ballots (match-any, one per bit of the digit); an entry's rank among them is popc(peers & lanes below),
//                   so equal digits keep their input order inside a chunk, chunks follow each other through the running offsets
//                   in LDS, and tiles through the scan: every pass is stable by construction, and so is the sort.
// It moves 12 bytes per entry and pass and is not tuned beyond that (no fused histograms).  A caller that knows digits to be the
// same in every key names the passes that matter (radix_sort_pairs_passes: pass_mask); a caller whose entry count is still on the
// device passes an upper bound as n and the address of the count as n_dev: tiles behind the count rank nothing.
// Entries: n < 2^32.  Workspace through dev_buf ("sort.hist", "sort.offs"); the caller brings the ping-pong pair.
#pragma once

#include <utility>

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

static constexpr uint32_t SORT_TILE = KMU_ANCHOR_SORT_TILE;
static_assert(SORT_TILE % 64 == 0, "a tile is walked in chunks of one wave");

// the lanes of `valid` whose 8-bit digit equals this lane's.  All 64 lanes must be active.
__device__ __forceinline__ uint64_t wave_match_digit(uint32_t d, uint64_t valid) {
    uint64_t peers = valid;
#pragma unroll
    for (int b = 0; b < 8; b++) {
        const bool bit = (d >> b) & 1u;
        const uint64_t v = __ballot(bit);
        peers &= bit ? v : ~v;
    }
    return peers;
}

static __global__ void __launch_bounds__(64) k_sort_hist(const uint64_t *keys, uint64_t n, const uint64_t *n_dev, uint32_t shift,
                                                         uint32_t n_tiles, uint32_t *hist) {
    __shared__ uint32_t h[256];
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    if (n_dev) n = min(n, *n_dev);
    for (uint32_t d = lane; d < 256; d += 64) h[d] = 0;
    __syncthreads();
    const uint64_t t0 = (uint64_t) tile * SORT_TILE;
    for (uint32_t c = 0; c < SORT_TILE; c += 64) {
        const uint64_t e = t0 + c + lane;
        if (e < n) atomicAdd(&h[(uint32_t) (keys[e] >> shift) & 255u], 1u);
    }
    __syncthreads();
    for (uint32_t d = lane; d < 256; d += 64) hist[(uint64_t) d * n_tiles + tile] = h[d];
}

static __global__ void __launch_bounds__(64) k_sort_scatter(const uint64_t *keys, const uint32_t *vals, uint64_t n,
                                                            const uint64_t *n_dev, uint32_t shift, uint32_t n_tiles,
                                                            const uint64_t *offs, uint64_t *keys_out, uint32_t *vals_out) {
    __shared__ uint32_t base[256]; // where the tile's next entry of every digit goes
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    if (n_dev) n = min(n, *n_dev);
    for (uint32_t d = lane; d < 256; d += 64) base[d] = (uint32_t) offs[(uint64_t) d * n_tiles + tile];
    __syncthreads();
    const uint64_t t0 = (uint64_t) tile * SORT_TILE;
    for (uint32_t c = 0; c < SORT_TILE; c += 64) { // uniform trip count: the ballots see all lanes
        const uint64_t e = t0 + c + lane;
        const bool valid = e < n;
        const uint64_t key = valid ? keys[e] : 0ull;
        const uint32_t val = valid ? vals[e] : 0u;
        const uint32_t d = (uint32_t) (key >> shift) & 255u;
        const uint64_t peers = wave_match_digit(d, __ballot(valid));
        const uint32_t rank = (uint32_t) __popcll(peers & ((1ull << lane) - 1ull));
        const uint32_t dst = base[d] + rank;
        __syncthreads(); // every lane has read its offset
        if (valid && (peers >> lane) == 1ull) base[d] = dst + 1; // the last lane of a digit moves its offset on
        __syncthreads();
        if (valid && dst < n) {
            keys_out[dst] = key;
            vals_out[dst] = val;
        }
    }
}

// Sorts the entries (k0[i], v0[i]) by the digits that pass_mask names (bit p: bits 8p .. 8p + 7 of the key), ascending; entries that
// agree in those digits keep their order.  n_dev == nullptr: n entries; otherwise min(n, *n_dev) of them, *n_dev device memory that
// earlier work on the stream has written.  (k1, v1) is scratch of the same size.  The pairs are swapped once per pass that runs, so on
// return (k0, v0) names the sorted entries and (k1, v1) the scratch.  All pointers are device memory; nothing is synchronised.
static inline int radix_sort_pairs_passes(kmu_ctx *ctx, uint64_t *&k0, uint32_t *&v0, uint64_t *&k1, uint32_t *&v1, uint64_t n,
                                          uint32_t pass_mask, const uint64_t *n_dev) {
    if (n == 0) return KMU_OK;
    if (n > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "radix_sort_pairs: %llu entries, more than 2^32 - 1", (unsigned long long) n);
    const uint32_t n_tiles = (uint32_t) ((n + SORT_TILE - 1) / SORT_TILE);
    uint64_t *offs;
    uint32_t *hist;
    KMU_TRY(dev_array(ctx, "sort.hist", (size_t) n_tiles * 256, &hist));
    KMU_TRY(dev_array(ctx, "sort.offs", (size_t) n_tiles * 256 + 1, &offs));
    for (uint32_t pass = 0; pass < 8; pass++) {
        if (!((pass_mask >> pass) & 1u)) continue;
        const uint32_t shift = 8 * pass;
        KMU_TRY(launch(ctx, "k_sort_hist", k_sort_hist, dim3(n_tiles), dim3(64), 0, (const uint64_t *) k0, n, n_dev, shift, n_tiles, hist));
        KMU_TRY(device_scan_u32(ctx, hist, (uint64_t) n_tiles * 256, offs));
        KMU_TRY(launch(ctx, "k_sort_scatter", k_sort_scatter, dim3(n_tiles), dim3(64), 0, (const uint64_t *) k0, (const uint32_t *) v0, n, n_dev,
                       shift, n_tiles, offs, k1, v1));
        std::swap(k0, k1);
        std::swap(v0, v1);
    }
    return KMU_OK;
}

// the pass_mask that can tell two ids below n apart: one bit per byte of n - 1 (at least the lowest)
static inline uint32_t radix_id_passes(uint32_t n) {
    uint32_t m = 1, top = n - 1;
    for (uint32_t b = 1; b < 4; b++)
        if (top >> (8 * b)) m |= 1u << b;
    return m;
}

// Sorts the n entries (k0[i], v0[i]) by key, ascending; entries of equal keys keep their order.  (k1, v1) is scratch of the same
// size; eight passes, so the sorted entries are back in (k0, v0).  All pointers are device memory; nothing is synchronised.
static inline int radix_sort_pairs(kmu_ctx *ctx, uint64_t *k0, uint32_t *v0, uint64_t *k1, uint32_t *v1, uint64_t n) {
    return radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n, 0xFFu, nullptr);
}

} // namespace kmu

// kmu_seed_tiles.h -- the two steps that the seed selectors of reads share (kmu_minimizers.hip, kmu_syncmers.hip): both cut the
// items of a read (windows of k-mers there, k-mer positions here) into tiles of 1024, deal one wave per tile and count per tile.
//  k_mini_tiles    one lane per read: its number of tiles (u32).  A read shorter than k has no tile and no k-mer that would look at
//                  its bases: its bytes are validated here.  device_scan_u32 makes the tile offsets tile_off[n_seq + 1].  With
//                  w = 1 a read's windows are its k-mers.
//  k_mini_offsets  out[i] = the offset of read i's first tile in the scanned per-tile counts: the first entry of read i.
#pragma once

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

static constexpr uint32_t MINI_T = KMU_MINIMIZER_TILE;
static_assert(KMU_SYNCMER_TILE == KMU_MINIMIZER_TILE, "both selectors count their tiles with k_mini_tiles");

// windows of a read of L bases: nk = L - k + 1 k-mers, max(nk - w, 0) + 1 windows if it has a k-mer at all
__host__ __device__ inline uint64_t mini_windows(uint64_t L, uint32_t k, uint32_t w) {
    if (L < k) return 0;
    const uint64_t nk = L - k + 1;
    return nk > w ? nk - w + 1 : 1;
}

static __global__ void __launch_bounds__(256) k_mini_tiles(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, uint32_t k, uint32_t w,
                                                           uint32_t *ntiles, uint32_t *err) {
    uint32_t bad = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += gridDim.x * blockDim.x) {
        const uint64_t beg = offsets[i], L = offsets[i + 1] - beg;
        ntiles[i] = (uint32_t) ((mini_windows(L, k, w) + MINI_T - 1) / MINI_T);
        if (L < k) // at most 31 bases
            for (uint64_t j = 0; j < L; j++) bad |= !is_acgt(bases[beg + j]);
    }
    if (bad) atomicOr(err, DERR_NON_ACGT);
}

static __global__ void __launch_bounds__(256) k_mini_offsets(const uint64_t *tile_off, const uint64_t *coff, uint32_t n_seq, uint64_t *out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i <= n_seq; i += (uint64_t) gridDim.x * blockDim.x)
        out[i] = coff[tile_off[i]];
}

} // namespace kmu

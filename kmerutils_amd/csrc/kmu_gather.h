// kmu_gather.h -- the segmented byte gather on the device: items of variable length become one contiguous byte stream plus 64-bit
// offsets (kmu_extract_ranges, kmu_sg_unitig_seqs; the arithmetic is in kmu_gather_core.h).
//
//  gather_find       the item that holds a wave-uniform byte: the 64-ary search of wave_find_read (kmu_flat.h) over a 64-bit index,
//                    since the number of items is a uint64, and over n + 1 entries; one probe per lane and trip, counted by ballot.
//  gather_tiles      one wave per tile of GATHER_TILE output bytes, 64 bytes per trip, one byte per lane, so the caller's stores are
//                    coalesced.  One long item spreads over many waves as many short ones share one.
//  k_gather_offsets  one lane per entry: the 64-bit offsets from the two 32-bit scans of the lengths' halves.
#pragma once

#include "kmu_device.h"
#include "kmu_gather_core.h"

namespace kmu {

// largest i in [0, n] with off[i] <= g, g wave-uniform
__device__ __forceinline__ uint64_t gather_find(const uint64_t *off, uint64_t n, uint64_t g) {
    const uint32_t lane = (uint32_t) lane_id();
    return gather_find_64ary(n, [&](uint64_t lo, uint64_t step, uint64_t hi) {
        const uint64_t idx = lo + (uint64_t) (lane + 1u) * step;
        return (uint32_t) __popcll(__ballot(idx < hi && off[idx] <= g));
    });
}

// ends: n_items + 1 ascending entries, ends[0] = 0, ends[n_items] = total.  Calls byte(r, o) once for every output byte o < total,
// with r < n_items and ends[r] <= o < ends[r + 1]; in a workgroup of 4 waves, tiles by grid stride
template <class Byte>
__device__ __forceinline__ void gather_tiles(const uint64_t *ends, uint64_t n_items, uint64_t total, uint64_t n_tiles, Byte byte) {
    const uint32_t lane = (uint32_t) lane_id();
    for (uint64_t t = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); t < n_tiles; t += (uint64_t) gridDim.x * 4u) {
        uint64_t pos = t * GATHER_TILE;
        const uint64_t tile_end = pos + GATHER_TILE < total ? pos + GATHER_TILE : total;
        uint64_t r0 = gather_find(ends, n_items, pos); // ends[r0] <= pos
        while (pos < tile_end) {
            // the window: the 64 ends behind r0, one per lane (beyond the last: never reached)
            const uint64_t wi = r0 + 1u + lane, win = wi <= n_items ? ends[wi] : ~0ull;
            const uint64_t w63 = ((uint64_t) readlane_u32((uint32_t) (win >> 32), 63) << 32) | readlane_u32((uint32_t) win, 63);
            if (w63 <= pos) { // 64 items that end at or before pos: empty ones
                r0 += 64u;
                continue;
            }
            uint64_t limit = pos + 64u < tile_end ? pos + 64u : tile_end;
            limit = w63 < limit ? w63 : limit; // (> pos) every byte below has its item inside the window
            const uint64_t o = pos + lane;
            const uint32_t c = gather_window_count(
                [&](uint32_t j) { return ((uint64_t) (uint32_t) __shfl((int) (win >> 32), (int) j, 64) << 32) | (uint32_t) __shfl((int) (uint32_t) win, (int) j, 64); }, o);
            if (o < limit) byte(r0 + c, o); // (c <= 63 and ends[r0 + c] <= o < ends[r0 + c + 1] <= total: r0 + c < n_items)
            r0 += (uint32_t) __popcll(__ballot(win <= limit));
            pos = limit;
        }
    }
}

static __global__ void __launch_bounds__(256) k_gather_offsets(const uint64_t *off_lo, const uint64_t *off_hi, uint64_t n, uint64_t *out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i <= n; i += (uint64_t) gridDim.x * blockDim.x)
        out[i] = off_lo[i] + (off_hi[i] << 32);
}

} // namespace kmu

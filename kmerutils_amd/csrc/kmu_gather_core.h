// kmu_gather_core.h -- the arithmetic of the segmented byte gather (kmu_gather.h): a list of variable-length items becomes one byte
// stream, item r at ends[r] .. ends[r + 1] (n + 1 ascending entries, ends[0] = 0; items may be empty).  The index of the item that
// holds a byte, for one lane and for a whole wave, a lane's item inside a window of 64 ends, and the tile size; for the device and
// for a host compiler alike (tests/cpp/sim_gather.h replays the tile walk from these functions over 64 simulated lanes).
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_GATHER_HD __host__ __device__ __forceinline__
#else
#define KMU_GATHER_HD inline
#endif

namespace kmu {

constexpr uint32_t GATHER_TILE = 4096; // output bytes per tile of the walk

// the largest i in [0, n] with off[i] <= g, off ascending with off[0] <= g: one lane's binary search.  Of equal entries it takes the
// last, so the item that holds byte g is never an empty one
KMU_GATHER_HD uint64_t gather_upper_index(const uint64_t *off, uint64_t n, uint64_t g) {
    uint64_t lo = 0, hi = n + 1u; // off[lo] <= g; off[hi] > g or hi == n + 1
    while (hi - lo > 1u) {
        const uint64_t mid = lo + (hi - lo) / 2u;
        if (off[mid] <= g) lo = mid;
        else hi = mid;
    }
    return lo;
}
// the same index for a whole wave, g wave-uniform: a 64-ary search over the n + 1 entries.  Lane l probes idx = lo + (l + 1) * step;
// count(lo, step, hi) is the number of lanes whose idx is below hi and has off[idx] <= g (a ballot and a population count on the
// device)
template <class Count> KMU_GATHER_HD uint64_t gather_find_64ary(uint64_t n, Count count) {
    uint64_t lo = 0, hi = n + 1u; // off[lo] <= g; off[hi] > g or hi == n + 1
    while (hi - lo > 1u) {
        const uint64_t step = (hi - lo + 63u) / 64u;
        const uint32_t c = count(lo, step, hi);
        const uint64_t nhi = lo + (uint64_t) (c + 1u) * step;
        lo += (uint64_t) c * step;
        hi = nhi < hi ? nhi : hi;
    }
    return lo;
}
// a lane's item inside a window of 64 ascending ends win[j] = ends[r0 + 1 + j]: the number of j with win[j] <= o, for a byte
// o < win[63].  get(j) returns win[j] (a wave shuffle on the device)
template <class Get> KMU_GATHER_HD uint32_t gather_window_count(Get get, uint64_t o) {
    uint32_t c = 0;
    for (uint32_t step = 32u; step >= 1u; step >>= 1)
        if (get(c + step - 1u) <= o) c += step;
    return c;
}

} // namespace kmu

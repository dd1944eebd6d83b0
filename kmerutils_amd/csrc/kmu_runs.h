// kmu_runs.h -- the step that kmu_anchor_overlaps.hip and kmu_seed_chains.hip share: from the flags "an inner unit begins at this
// sorted entry" (a run of one diagonal there, a group of one strand here) and "a read pair begins at this entry", and their
// exclusive scans, to the first entry of every inner unit and the first inner unit of every read pair.
#pragma once

#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

struct RunMarks {
    const uint64_t *n_dev;        // the number of entries, on the device
    uint64_t n_max;               // its upper bound: the size of the flag arrays
    const uint32_t *rhead, *phead;
    const uint64_t *ridx, *pidx;  // exclusive scans of the flags; [n_max] = inner units, read pairs
    uint32_t *rstart, *pstart;    // first entry of unit r (and n behind the last); first unit of read pair q (and the units behind the last)
};

static __global__ void __launch_bounds__(256) k_run_starts(RunMarks m) {
    const uint64_t n = min(*m.n_dev, m.n_max);
    const uint64_t first = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = first; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        if (m.rhead[i]) m.rstart[m.ridx[i]] = (uint32_t) i;
        if (m.phead[i]) m.pstart[m.pidx[i]] = (uint32_t) m.ridx[i];
    }
    if (first == 0) {
        m.rstart[m.ridx[m.n_max]] = (uint32_t) n;
        m.pstart[m.pidx[m.n_max]] = (uint32_t) m.ridx[m.n_max];
    }
}

} // namespace kmu

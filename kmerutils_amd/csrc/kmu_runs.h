// kmu_runs.h -- from matched pairs to "entries sorted by (read_a, read_b, inner key), flagged, scanned, with starts": the grouping that
// kmu_anchor_overlaps.hip (an entry is one strand of a window pair, the inner unit a run of one diagonal) and kmu_seed_chains.hip
// (an entry is an anchor, the inner unit a group of one strand) share, and every step that produces it.  A unit embeds one PairRuns
// as the member `r` of its argument block and brings a policy struct U of three static device functions:
//   bool     U::decode(a, p, item, bad)  pair p: does it survive; what the unit keeps of it in registers (U::Item); a pair that the
//                                        call cannot take sets bad and has to come back harmless
//   void     U::store(a, p, c, item)     survivor c: the unit's per-survivor arrays, r.prim[c], and the r.per entries
//                                        o = c * r.per .. of r.skeys (the inner sort key) and r.svals (o)
//   uint64_t U::inner(a, v)              the inner key of the sorted value v: where it changes inside a read pair, a unit begins
//
//  runs_compact    the body of the unit's k_*_keys<WRITE>.  One wave per tile of SORT_TILE pairs, one lane per pair: decode,
//                  survivors compacted in lane order by ballot and prefix count, store.  COUNT leaves one count per tile and
//                  device_scan_u32 makes the offsets; where every pair survives COUNT is not run.  The number of entries stays
//                  on the device (RunInfo::n): every later kernel and the sort read it there, sized by the host's n_max.
//  k_run_gather    the read pair of every entry in the place the first sort gave it.
//  k_run_heads     one lane per sorted entry: does the inner unit change here, does the read pair change here; keep = 0.
//  k_run_starts    the first entry of every inner unit and the first inner unit of every read pair.
// and the host steps, in the order a call takes them: runs_workspace, runs_keys, runs_order, (the unit's walk over the inner units
// and its COUNT over the read pairs, which leaves r.keep), runs_total, runs_emit.  A kernel is profiled under the unit's name,
// k_<unit>_<step>.  The workspace is one set of arrays for both units ("runs.*"): nothing of a call outlives it.
#pragma once

#include "kmu_sort.h"

namespace kmu {

struct RunInfo {
    uint64_t n;   // entries: survivors * per
    uint32_t bad; // the call is refused at its synchronisation.  runs_workspace zeroes it, kernels only OR into it
    uint32_t pad;
};

struct PairRuns {
    RunInfo *info;
    uint64_t n_pairs;
    uint64_t n_max;      // n_pairs * per: the size every per-entry array has
    uint32_t per, shift; // entries per survivor; sorted value >> shift = its survivor
    uint32_t n_tiles;    // tiles of SORT_TILE pairs
    uint32_t *counts;    // survivors per tile
    uint64_t *coff;      // their exclusive scan; null where every pair survives
    uint64_t *prim; // per survivor c: read_a << 32 | read_b
    // per entry: the inner keys, then (runs_order) the read pairs, sorted; the entry numbers; the sort's other pair
    uint64_t *skeys, *keys1;
    uint32_t *svals, *vals1;
    uint32_t *rhead, *phead, *keep;
    uint64_t *ridx, *pidx;     // exclusive scans of the flags; [n_max] = inner units, read pairs
    uint32_t *rstart, *pstart; // first entry of unit r (and n behind the last); first unit of read pair q (and the units behind the last)
    uint64_t *ooff;            // exclusive scan of keep; [n_max] = records
    uint64_t total;
};

template <class U, bool WRITE, class Args> __device__ __forceinline__ void runs_compact(const Args &a) {
    const PairRuns &r = a.r;
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t t0 = (uint64_t) tile * SORT_TILE;
    uint64_t at = WRITE ? (r.coff ? r.coff[tile] : t0) : 0ull; // where the tile's next survivor goes / how many it keeps so far
    if (WRITE && tile == 0 && lane == 0) r.info->n = (r.coff ? r.coff[r.n_tiles] : r.n_pairs) * r.per;
    uint32_t bad = 0;
    for (uint32_t c0 = 0; c0 < SORT_TILE; c0 += 64) { // uniform trip count: all lanes reach the ballot
        const uint64_t p = t0 + c0 + lane;
        typename U::Item item{};
        const bool pass = p < r.n_pairs && U::decode(a, p, item, bad);
        const uint64_t bal = __ballot(pass);
        if (WRITE) {
            const uint64_t c = at + (uint64_t) __popcll(bal & below);
            if (pass && c < r.n_pairs) U::store(a, p, c, item);
        }
        at += (uint64_t) __popcll(bal);
    }
    if (!WRITE && lane == 0) r.counts[tile] = (uint32_t) at;
    if (WRITE && bad) atomicOr(&r.info->bad, 1u);
}

static __global__ void __launch_bounds__(256) k_run_gather(PairRuns r) {
    const uint64_t n = min(r.info->n, r.n_max);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        r.skeys[i] = r.prim[r.svals[i] >> r.shift];
}

// behind the last entry the flags are 0, and so is every keep
template <class U, class Args> static __global__ void __launch_bounds__(256) k_run_heads(Args a) {
    const PairRuns &r = a.r;
    const uint64_t n = min(r.info->n, r.n_max);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < r.n_max; i += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t rh = 0, ph = 0;
        if (i < n) {
            ph = i == 0 || r.skeys[i] != r.skeys[i - 1];
            rh = ph || U::inner(a, r.svals[i]) != U::inner(a, r.svals[i - 1]);
        }
        r.rhead[i] = rh;
        r.phead[i] = ph;
        r.keep[i] = 0;
    }
}

static __global__ void __launch_bounds__(256) k_run_starts(PairRuns r) {
    const uint64_t n = min(r.info->n, r.n_max);
    const uint64_t first = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = first; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        if (r.rhead[i]) r.rstart[r.ridx[i]] = (uint32_t) i;
        if (r.phead[i]) r.pstart[r.pidx[i]] = (uint32_t) r.ridx[i];
    }
    if (first == 0) {
        r.rstart[r.ridx[r.n_max]] = (uint32_t) n;
        r.pstart[r.pidx[r.n_max]] = (uint32_t) r.ridx[r.n_max];
    }
}

// "k_<unit>_<step>": the name a shared kernel is profiled under
struct RunName {
    char s[32];
    RunName(const char *unit, const char *step) { snprintf(s, sizeof s, "k_%s_%s", unit, step); }
};

// the common arrays of a call of n_pairs pairs, `per` entries each, and a clean info.  `count`: not every pair survives
static inline int runs_workspace(kmu_ctx *ctx, PairRuns &r, uint64_t n_pairs, uint32_t per, uint32_t shift, bool count) {
    const uint64_t n_max = n_pairs * per;
    r.n_pairs = n_pairs;
    r.n_max = n_max;
    r.per = per;
    r.shift = shift;
    r.n_tiles = (uint32_t) ((n_pairs + SORT_TILE - 1) / SORT_TILE);
    KMU_TRY(dev_array(ctx, "runs.info", 1, &r.info));
    KMU_TRY(dev_array(ctx, "runs.counts", r.n_tiles, &r.counts));
    KMU_TRY(dev_array(ctx, "runs.coff", (size_t) r.n_tiles + 1, &r.coff));
    KMU_TRY(dev_array(ctx, "runs.prim", n_pairs, &r.prim));
    KMU_TRY(dev_array(ctx, "runs.keys0", n_max, &r.skeys));
    KMU_TRY(dev_array(ctx, "runs.vals0", n_max, &r.svals));
    KMU_TRY(dev_array(ctx, "runs.keys1", n_max, &r.keys1));
    KMU_TRY(dev_array(ctx, "runs.vals1", n_max, &r.vals1));
    KMU_TRY(dev_array(ctx, "runs.rhead", n_max, &r.rhead));
    KMU_TRY(dev_array(ctx, "runs.phead", n_max, &r.phead));
    KMU_TRY(dev_array(ctx, "runs.keep", n_max, &r.keep));
    KMU_TRY(dev_array(ctx, "runs.ridx", (size_t) n_max + 1, &r.ridx));
    KMU_TRY(dev_array(ctx, "runs.pidx", (size_t) n_max + 1, &r.pidx));
    KMU_TRY(dev_array(ctx, "runs.ooff", (size_t) n_max + 1, &r.ooff));
    KMU_TRY(dev_array(ctx, "runs.rstart", (size_t) n_max + 1, &r.rstart));
    KMU_TRY(dev_array(ctx, "runs.pstart", (size_t) n_max + 1, &r.pstart));
    if (!count) r.coff = nullptr;
    KMU_HIP(ctx, hipMemsetAsync(r.info, 0, sizeof(RunInfo), ctx->stream));
    return KMU_OK;
}

// the unit's two instantiations of runs_compact: COUNT and the scan of its counts where not every pair survives, WRITE
template <class Args> static inline int runs_keys(kmu_ctx *ctx, const char *unit, const Args &a, void (*count)(Args), void (*write)(Args)) {
    const PairRuns &r = a.r;
    if (r.coff) {
        KMU_TRY(launch(ctx, RunName(unit, "keys_count").s, count, dim3(r.n_tiles), dim3(64), 0, a));
        KMU_TRY(device_scan_u32(ctx, r.counts, r.n_tiles, r.coff));
    }
    return launch(ctx, RunName(unit, "keys_write").s, write, dim3(r.n_tiles), dim3(64), 0, a);
}

// by the inner key (the passes of inner_passes), then (stable) by read pair: only the bytes that n_reads_q and n_reads_db can
// reach; then flags, their scans and the starts.  Leaves a.r as the kernels behind it read it.
template <class U, class Args>
static inline int runs_order(kmu_ctx *ctx, const char *unit, Args &a, uint32_t inner_passes, uint32_t n_reads_q, uint32_t n_reads_db) {
    PairRuns &r = a.r;
    const uint32_t flat = grid_for(ctx, r.n_max, 256);
    KMU_TRY(radix_sort_pairs_passes(ctx, r.skeys, r.svals, r.keys1, r.vals1, r.n_max, inner_passes, &r.info->n));
    KMU_TRY(launch(ctx, RunName(unit, "gather").s, k_run_gather, dim3(flat), dim3(256), 0, r));
    KMU_TRY(radix_sort_pairs_passes(ctx, r.skeys, r.svals, r.keys1, r.vals1, r.n_max,
                                    radix_id_passes(n_reads_db) | (radix_id_passes(n_reads_q) << 4), &r.info->n));
    KMU_TRY(launch(ctx, RunName(unit, "heads").s, k_run_heads<U, Args>, dim3(flat), dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, r.rhead, r.n_max, r.ridx));
    KMU_TRY(device_scan_u32(ctx, r.phead, r.n_max, r.pidx));
    return launch(ctx, RunName(unit, "starts").s, k_run_starts, dim3(flat), dim3(256), 0, r);
}

// From r.keep to the number of records, with the call's one synchronisation.  *emit: there are records and the caller has room
// for them (r.total); otherwise the call is over and the return value is its own: refused (`refusal`), counted, empty, or too
// many `noun` for cap.
static inline int runs_total(kmu_ctx *ctx, PairRuns &r, int mem, bool writing, uint64_t cap, uint64_t *n_out, const char *noun,
                             const char *refusal, bool *emit) {
    *emit = false;
    KMU_TRY(device_scan_u32(ctx, r.keep, r.n_max, r.ooff));
    RunInfo h_info{};
    KMU_TRY(read_back(ctx, {{&r.total, r.ooff + r.n_max}, {&h_info, r.info}}));
    if (h_info.bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED, "%s", refusal);
    }
    *n_out = r.total;
    if (!writing || r.total == 0) return finish_call(ctx, mem);
    if (cap < r.total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu %s, room for %llu", (unsigned long long) r.total, noun, (unsigned long long) cap);
    }
    *emit = true;
    return KMU_OK;
}

// the r.total records: write(where) launches the unit's WRITE kernel; a host caller's records pass through the workspace
template <class T, class Write> static inline int runs_emit(kmu_ctx *ctx, const PairRuns &r, int mem, T *out, Write write) {
    T *dev;
    KMU_TRY(place_output(ctx, "runs.out", out, r.total, mem, &dev));
    KMU_TRY(write(dev));
    KMU_TRY(bring_output(ctx, out, dev, r.total, mem));
    return finish_call(ctx, mem);
}

} // namespace kmu

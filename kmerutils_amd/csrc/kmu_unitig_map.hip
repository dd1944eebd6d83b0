// kmu_unitig_map.hip -- one chain record per read saying where the read lies on which unitig: from the layout for a read on a path,
// from the read's containment record projected through the container's place for a contained read (kmu_sg_unitig_chains; the
// contract is in include/kmu.h, the arithmetic in kmu_um_core.h).  Every kernel is a flat grid-stride loop; the launch count does
// not depend on the data.
//
//  k_um_check  one lane per unitig, per step and per place: the checks of the contract; a place checks every record it names
//              before it uses it as an index, so the three loops need no order.
//  Every later kernel returns at once where bad is raised: a refused call leaves its outputs untouched also in device memory, and
//  nothing reads a layout that failed a check.
//  k_um_cand   one lane per chain record: a record of class A_CONTAINED / B_CONTAINED passes its range checks first (one that
//              fails raises bad and is never used as an index), then candidacy, then one 64-bit atomic maximum at its contained read.
//  k_um_flag   one lane per read: 1 where the read has a record; counts n_layout and n_contained.
//  (device_scan_u32 over the reads)
//  k_um_write  one lane per read: its record, rebuilt from the place or from the winning chain record.
#include <string.h>

#include "kmu_ctx.hpp"
#include "kmu_um_core.h"

namespace kmu {

enum { UM_LAYOUT, UM_CONTAINED }; // counters behind kmu_um_stats

struct UmArgs {
    const kmu_sg_unitig *unitigs;
    uint64_t n_unitigs;
    const kmu_sg_step *path;
    uint64_t n_steps;
    const kmu_sg_place *place;
    const kmu_chain *chains;
    const uint8_t *classes;
    uint64_t n_chains;
    const uint64_t *off;
    uint32_t n_reads;
    unsigned long long *stats; // 2 counters, start as 0
    unsigned long long *best;  // per read, starts as 0: the key of the winning candidate
    uint32_t *bad;             // kernels only store 1 to it
    uint32_t *has;             // per read
    const uint64_t *pos;       // the scan of has
    kmu_chain *out;
};

#define UM_FOR(i, n) for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t) gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) k_um_check(UmArgs a) {
    bool bad = false;
    UM_FOR(u, a.n_unitigs) bad |= !um_unitig_ok(a.unitigs[u], a.n_steps);
    UM_FOR(i, a.n_steps) bad |= !um_step_ok(a.path[i], a.n_reads);
    UM_FOR(r, a.n_reads) bad |= !um_place_ok(a.unitigs, a.n_unitigs, a.path, a.n_steps, a.place[r], (uint32_t) r);
    if (bad) *a.bad = 1u;
}

__global__ void __launch_bounds__(256) k_um_cand(UmArgs a) {
    if (*a.bad) return;
    bool bad = false;
    UM_FOR(x, a.n_chains) {
        const uint32_t cls = a.classes[x];
        if (!um_is_containment(cls)) continue;
        const kmu_chain rec = a.chains[x];
        if (!um_rec_reads_ok(rec, a.n_reads) ||
            !um_rec_segs_ok(rec, a.off[rec.read_a + 1u] - a.off[rec.read_a], a.off[rec.read_b + 1u] - a.off[rec.read_b])) {
            bad = true;
            continue;
        }
        const UmCand k = um_cand(rec, cls);
        if (a.place[k.c].unitig != KMU_SG_NONE) continue;
        const kmu_sg_place pg = a.place[k.g];
        if (pg.unitig == KMU_SG_NONE) continue;
        const uint64_t e_g = a.path[a.unitigs[pg.unitig].first + pg.rank].end; // (the place has passed k_um_check)
        if (um_project(k, pg.strand, e_g, a.off[k.g + 1u] - a.off[k.g]) < 0) continue;
        atomicMax(&a.best[k.c], um_key(k, x));
    }
    if (bad) *a.bad = 1u;
}

__global__ void __launch_bounds__(256) k_um_flag(UmArgs a) {
    if (*a.bad) return;
    uint32_t n_layout = 0, n_contained = 0;
    UM_FOR(r, a.n_reads) {
        const bool layout = a.place[r].unitig != KMU_SG_NONE, contained = !layout && a.best[r] != 0ull;
        a.has[r] = layout || contained;
        n_layout += layout;
        n_contained += contained;
    }
    if (n_layout) atomicAdd(&a.stats[UM_LAYOUT], (unsigned long long) n_layout);
    if (n_contained) atomicAdd(&a.stats[UM_CONTAINED], (unsigned long long) n_contained);
}

__global__ void __launch_bounds__(256) k_um_write(UmArgs a) {
    if (*a.bad) return;
    UM_FOR(r, a.n_reads) {
        if (!a.has[r]) continue;
        const kmu_sg_place p = a.place[r];
        kmu_chain c;
        if (p.unitig != KMU_SG_NONE) {
            const uint64_t e = a.path[a.unitigs[p.unitig].first + p.rank].end;
            c = um_layout_record(p.unitig, (uint32_t) r, p.strand, e, a.off[r + 1u] - a.off[r]);
        } else {
            const uint32_t x = um_key_index(a.best[r]);
            const kmu_chain rec = a.chains[x];
            const UmCand k = um_cand(rec, a.classes[x]);
            const kmu_sg_place pg = a.place[k.g];
            const uint64_t e_g = a.path[a.unitigs[pg.unitig].first + pg.rank].end;
            c = um_contained_record(k, x, rec.strand, pg.unitig, pg.strand, um_project(k, pg.strand, e_g, a.off[k.g + 1u] - a.off[k.g]));
        }
        a.out[a.pos[r]] = c;
    }
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_sg_unitig_chains(kmu_ctx *ctx, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path, uint64_t n_steps,
                                    const kmu_sg_place *place, const kmu_chain *chains, const uint8_t *classes, uint64_t n_chains,
                                    const uint64_t *offsets, uint32_t n_reads, const kmu_um_params *p, int mem, kmu_chain *out,
                                    kmu_um_stats *stats_out, uint64_t *n_out) {
    // (the arguments are judged before the context is needed: fail() keeps the message of a call without one)
    if (!p || !offsets || !stats_out || !n_out || (!unitigs && n_unitigs) || (!path && n_steps) || ((!place || !out) && n_reads) ||
        ((!chains || !classes) && n_chains))
        return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags || p->zero) return fail(ctx, KMU_E_BAD_ARG, "flags = 0x%x and zero = %u must be 0", p->flags, p->zero);
    KMU_TRY(check_mem(ctx, mem));
    if (n_reads >= 0x80000000u) return fail(ctx, KMU_E_UNSUPPORTED, "%u reads: 2^31 or more", n_reads);
    if (n_chains >= 0x100000000ull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu chains: 2^32 or more", (unsigned long long) n_chains);
    if (!ctx) return fail(ctx, KMU_E_BAD_ARG, "null context");
    if (n_reads == 0) {
        *stats_out = kmu_um_stats{};
        *n_out = 0;
        return KMU_OK;
    }
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    UmArgs a{};
    KMU_TRY(stage_to_device(ctx, "um.unitigs", unitigs, (size_t) n_unitigs, mem, &a.unitigs));
    a.n_unitigs = n_unitigs;
    KMU_TRY(stage_to_device(ctx, "um.path", path, (size_t) n_steps, mem, &a.path));
    a.n_steps = n_steps;
    KMU_TRY(stage_to_device(ctx, "um.place", place, (size_t) n_reads, mem, &a.place));
    KMU_TRY(stage_to_device(ctx, "um.chains", chains, (size_t) n_chains, mem, &a.chains));
    KMU_TRY(stage_to_device(ctx, "um.classes", classes, (size_t) n_chains, mem, &a.classes));
    a.n_chains = n_chains;
    KMU_TRY(stage_to_device(ctx, "um.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;

    // the workspace: the two counters, the keys (8-byte aligned, start as 0) and the refusal flag behind them; the flags and their scan
    const size_t n_zero = 2 + (size_t) n_reads + 1;
    unsigned long long *zeros;
    uint64_t *pos;
    KMU_TRY(dev_array(ctx, "um.zeros", n_zero, &zeros));
    KMU_TRY(dev_array(ctx, "um.has", n_reads, &a.has));
    KMU_TRY(dev_array(ctx, "um.pos", (size_t) n_reads + 1, &pos));
    a.stats = zeros;
    a.best = zeros + 2;
    a.bad = (uint32_t *) (zeros + 2 + n_reads);
    a.pos = pos;
    KMU_TRY(place_output(ctx, "um.out", out, n_reads, mem, &a.out));
    KMU_HIP(ctx, hipMemsetAsync(zeros, 0, n_zero * 8, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.has, 0, (size_t) n_reads * 4, ctx->stream));

    const dim3 per_read(grid_for(ctx, n_reads, 256)), block(256);
    const uint64_t n_check = std::max<uint64_t>(std::max<uint64_t>(n_unitigs, n_steps), n_reads);
    KMU_TRY(launch(ctx, "k_um_check", k_um_check, dim3(grid_for(ctx, n_check, 256)), block, 0, a));
    KMU_TRY(launch(ctx, "k_um_cand", k_um_cand, dim3(grid_for(ctx, n_chains, 256)), block, 0, a));
    KMU_TRY(launch(ctx, "k_um_flag", k_um_flag, per_read, block, 0, a));
    KMU_TRY(device_scan_u32(ctx, a.has, n_reads, pos));
    KMU_TRY(launch(ctx, "k_um_write", k_um_write, per_read, block, 0, a));

    // the counts and the refusal flag come to the host (the synchronisation)
    unsigned long long h_stats[2] = {0, 0};
    uint64_t n_rec = 0;
    uint32_t h_bad = 0;
    KMU_TRY(read_back(ctx, {{h_stats, a.stats, sizeof h_stats}, {&n_rec, pos + n_reads}, {&h_bad, a.bad}}));
    if (h_bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED,
                    "a unitig's steps lie outside the step list or its len is 2^32 or more, a step names a read that does not exist, a "
                    "strand above 1 or an end of 0, a place does not match its unitig and step, or a containment record names a read "
                    "that does not exist, a strand above 1 or a segment outside its read");
    }
    stats_out->n_layout = h_stats[UM_LAYOUT];
    stats_out->n_contained = h_stats[UM_CONTAINED];
    stats_out->n_unplaced = (uint64_t) n_reads - h_stats[UM_LAYOUT] - h_stats[UM_CONTAINED];
    *n_out = n_rec;
    KMU_TRY(bring_output(ctx, out, a.out, n_rec, mem));
    return finish_call(ctx, mem);
}

// kmu_clean.hip -- string graph cleaning on the resident arcs: short dead ends (tips) are removed, simple bubbles are popped, unique
// and the degrees are recomputed (kmu_sg_clean; the contract is in include/kmu.h, the arithmetic in kmu_clean_core.h).  Every kernel
// is a flat grid-stride loop; the launch count does not depend on the graph.
//
//  k_cl_check    one lane per arc: `from` must not decrease (every arc: the searches run over all of them); a surviving arc passes
//                the range checks first (one that fails raises bad and is never used as an index), then the mate search and the
//                contained test; integer atomics count deg1[from] and keep the smallest `to` in sole1[from].
//  Every later kernel returns at once where bad is raised: a refused call leaves its outputs untouched also in device memory, and
//  nothing walks a graph that failed a check.
//  k_cl_tips     one lane per vertex: the walk of a tip start; a candidate publishes its read count at its last vertex (one writer:
//                the walk backwards from a last vertex is unique).
//  k_cl_spare    one lane per junction: where every in-neighbour ends a candidate, the one the contract names is spared.
//  k_cl_tipkill  one lane per tip start, walking again: the reads of a candidate that is not spared get KMU_SG_READ_TIP.
//  k_cl_flag     one lane per arc, launched once per phase: the arc goes to arcs_out with the phase's flag where it touches a flagged
//                read; the degrees and sole of the arcs that still survive are counted again.
//  k_cl_bubbles  one lane per source: both branches are walked (two registers each: no scratch), the loser is walked AGAIN to flag
//                its reads.  s and t ^ 1 store the same bits.
//  k_cl_unique   one lane per arc: unique from the final degrees, the arcs that are left.
//  k_cl_reads    one lane per read: the summary with the new flag bits and the final degrees.
#include <string.h>

#include "kmu_clean_core.h"
#include "kmu_ctx.hpp"

namespace kmu {

enum { CL_TIPS, CL_TIP_READS, CL_SPARED, CL_BUBBLES, CL_BUBBLE_READS, CL_ARCS_TIP, CL_ARCS_BUBBLE, CL_ARCS_LEFT }; // kmu_sg_clean_stats

struct ClArgs {
    const kmu_sg_arc *arcs;
    uint64_t n_arcs;
    const kmu_sg_read *reads; // or null
    uint32_t n_reads, T, B;
    uint32_t *deg1, *deg2, *deg3; // per vertex, start as 0
    uint32_t *sole1, *sole2;      // per vertex, start as KMU_SG_NONE
    uint32_t *tipcnt, *spared;    // per vertex, start as 0
    uint32_t *rflag;              // per read, start as 0: the new flag bits
    unsigned long long *stats;    // 8 counters
    uint32_t *bad;                // kernels only store 1 to it
    kmu_sg_arc *arcs_out;
    kmu_sg_read *reads_out; // or null
};

#define CL_FOR(i, n) for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < (n); i += (uint64_t) gridDim.x * blockDim.x)

__global__ void __launch_bounds__(256) k_cl_check(ClArgs a) {
    bool bad = false;
    CL_FOR(i, a.n_arcs) {
        const kmu_sg_arc x = a.arcs[i];
        if (i && x.from < a.arcs[i - 1u].from) bad = true;
        if (!cl_survives(x)) continue;
        bool ok = cl_arc_ok(x, a.n_reads);
        if (ok && a.reads) ok = !((a.reads[x.from >> 1].flags | a.reads[x.to >> 1].flags) & KMU_SG_READ_CONTAINED);
        if (ok) ok = cl_has_mate(a.arcs, a.n_arcs, x);
        if (ok) {
            atomicAdd(&a.deg1[x.from], 1u);
            atomicMin(&a.sole1[x.from], x.to);
        }
        bad |= !ok;
    }
    if (bad) *a.bad = 1u;
}

__global__ void __launch_bounds__(256) k_cl_tips(ClArgs a) {
    if (*a.bad || a.T == 0u) return;
    CL_FOR(v, 2ull * a.n_reads) {
        const ClTip t = cl_tip_walk(a.deg1, a.sole1, (uint32_t) v, a.T);
        if (t.cnt) a.tipcnt[t.last] = t.cnt;
    }
}

__global__ void __launch_bounds__(256) k_cl_spare(ClArgs a) {
    if (*a.bad || a.T == 0u) return;
    uint32_t n = 0;
    CL_FOR(w, 2ull * a.n_reads) {
        const uint32_t u = cl_spared(a.arcs, a.n_arcs, a.deg1, a.tipcnt, (uint32_t) w);
        if (u == KMU_SG_NONE) continue;
        a.spared[u] = 1u;
        n++;
    }
    if (n) atomicAdd(&a.stats[CL_SPARED], (unsigned long long) n);
}

__global__ void __launch_bounds__(256) k_cl_tipkill(ClArgs a) {
    if (*a.bad || a.T == 0u) return;
    uint32_t tips = 0, tip_reads = 0;
    CL_FOR(v0, 2ull * a.n_reads) {
        const ClTip t = cl_tip_walk(a.deg1, a.sole1, (uint32_t) v0, a.T);
        if (!t.cnt || a.spared[t.last]) continue;
        uint32_t v = (uint32_t) v0;
        for (uint32_t i = 0; i < t.cnt; i++, v = a.sole1[v]) atomicOr(&a.rflag[v >> 1], KMU_SG_READ_TIP);
        tips++;
        tip_reads += t.cnt;
    }
    if (tips) {
        atomicAdd(&a.stats[CL_TIPS], (unsigned long long) tips);
        atomicAdd(&a.stats[CL_TIP_READS], (unsigned long long) tip_reads);
    }
}

// src: the input arcs in phase 1, arcs_out itself in phase 2 (every lane reads and writes its own arc only)
__global__ void __launch_bounds__(256) k_cl_flag(ClArgs a, const kmu_sg_arc *src, uint32_t bit, uint32_t *deg, uint32_t *sole, int stat,
                                                 int stat_left) {
    if (*a.bad) return;
    uint32_t flagged = 0, left = 0;
    CL_FOR(i, a.n_arcs) {
        const kmu_sg_arc x = src[i];
        uint32_t flags = x.flags;
        if (cl_survives(x)) { // (a surviving arc has passed the checks)
            flags = cl_arc_flag(a.rflag[x.from >> 1], a.rflag[x.to >> 1], bit);
            if (flags) {
                flagged++;
            } else {
                left++;
                atomicAdd(&deg[x.from], 1u);
                if (sole) atomicMin(&sole[x.from], x.to);
            }
        }
        a.arcs_out[i] = kmu_sg_arc{x.from, x.to, x.len, x.ovl, x.rec, flags, 0u, x.zero}; // (a changed copy of x goes through LDS)
    }
    if (flagged) atomicAdd(&a.stats[stat], (unsigned long long) flagged);
    if (left && stat_left >= 0) atomicAdd(&a.stats[stat_left], (unsigned long long) left);
}

__global__ void __launch_bounds__(256) k_cl_bubbles(ClArgs a) {
    if (*a.bad || a.B == 0u) return;
    uint32_t bubbles = 0, bubble_reads = 0;
    CL_FOR(s, 2ull * a.n_reads) {
        const ClBubble b = cl_bubble(a.arcs_out, a.n_arcs, a.deg2, a.sole2, (uint32_t) s, a.B);
        if (!b.k) continue;
        uint32_t v = b.first;
        for (uint32_t i = 0; i < b.k; i++, v = a.sole2[v]) atomicOr(&a.rflag[v >> 1], KMU_SG_READ_BUBBLE);
        if (cl_bubble_counts((uint32_t) s, b.t)) {
            bubbles++;
            bubble_reads += b.k;
        }
    }
    if (bubbles) {
        atomicAdd(&a.stats[CL_BUBBLES], (unsigned long long) bubbles);
        atomicAdd(&a.stats[CL_BUBBLE_READS], (unsigned long long) bubble_reads);
    }
}

__global__ void __launch_bounds__(256) k_cl_unique(ClArgs a) {
    if (*a.bad) return;
    CL_FOR(i, a.n_arcs) {
        const kmu_sg_arc x = a.arcs_out[i];
        if (cl_unique(x, a.deg3)) a.arcs_out[i].unique = 1u;
    }
}

__global__ void __launch_bounds__(256) k_cl_reads(ClArgs a) {
    if (*a.bad || !a.reads_out) return;
    CL_FOR(r, a.n_reads) {
        kmu_sg_read x = a.reads ? a.reads[r] : kmu_sg_read{0u, 0u, 0u, 0u};
        x.flags |= a.rflag[r];
        x.out_fwd = a.deg3[2u * r];
        x.out_rev = a.deg3[2u * r + 1u];
        a.reads_out[r] = x;
    }
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_sg_clean(kmu_ctx *ctx, const kmu_sg_arc *arcs, uint64_t n_arcs, const kmu_sg_read *reads, uint32_t n_reads,
                            const kmu_sg_clean_params *p, int mem, kmu_sg_arc *arcs_out, kmu_sg_read *reads_out,
                            kmu_sg_clean_stats *stats_out) {
    // (the arguments are judged before the context is needed: fail() keeps the message of a call without one)
    if (!p || !stats_out || ((!arcs || !arcs_out) && n_arcs)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags || p->zero) return fail(ctx, KMU_E_BAD_ARG, "flags = 0x%x and zero = %u must be 0", p->flags, p->zero);
    if (p->max_tip_reads > KMU_SG_CLEAN_MAX || p->max_bubble_reads > KMU_SG_CLEAN_MAX)
        return fail(ctx, KMU_E_BAD_ARG, "max_tip_reads = %u, max_bubble_reads = %u: at most %u", p->max_tip_reads, p->max_bubble_reads,
                    KMU_SG_CLEAN_MAX);
    KMU_TRY(check_mem(ctx, mem));
    if (n_reads >= 0x80000000u) return fail(ctx, KMU_E_UNSUPPORTED, "%u reads: 2^31 or more", n_reads);
    if (n_arcs >= 0x100000000ull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu arcs: 2^32 or more", (unsigned long long) n_arcs);
    if (n_arcs && !n_reads) return fail(ctx, KMU_E_BAD_ARG, "arcs but no reads");
    if (n_arcs) {
        const uintptr_t in = (uintptr_t) arcs, out = (uintptr_t) arcs_out, bytes = (uintptr_t) n_arcs * sizeof(kmu_sg_arc);
        if (in < out + bytes && out < in + bytes) return fail(ctx, KMU_E_BAD_ARG, "arcs_out overlaps arcs");
    }
    if (!ctx) return fail(ctx, KMU_E_BAD_ARG, "null context");
    if (n_reads == 0) {
        *stats_out = kmu_sg_clean_stats{};
        return KMU_OK;
    }
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    ClArgs a{};
    KMU_TRY(stage_to_device(ctx, "cl.arcs", arcs, (size_t) n_arcs, mem, &a.arcs));
    a.n_arcs = n_arcs;
    KMU_TRY(stage_to_device(ctx, "cl.reads", reads, (size_t) n_reads, mem, &a.reads));
    a.n_reads = n_reads;
    a.T = p->max_tip_reads;
    a.B = p->max_bubble_reads;

    // the workspace: counters and flags (start as 0; the stats first, 8-byte aligned), sole (starts as KMU_SG_NONE)
    const size_t n_v = 2 * (size_t) n_reads, n_zero = 16 + 2 + 5 * n_v + n_reads;
    uint32_t *zeros;
    KMU_TRY(dev_array(ctx, "cl.zeros", n_zero, &zeros));
    KMU_TRY(dev_array(ctx, "cl.sole", 2 * n_v, &a.sole1));
    a.stats = (unsigned long long *) zeros;
    a.bad = zeros + 16;
    a.deg1 = zeros + 18;
    a.deg2 = a.deg1 + n_v;
    a.deg3 = a.deg2 + n_v;
    a.tipcnt = a.deg3 + n_v;
    a.spared = a.tipcnt + n_v;
    a.rflag = a.spared + n_v;
    a.sole2 = a.sole1 + n_v;
    KMU_TRY(place_output(ctx, "cl.out", arcs_out, n_arcs ? n_arcs : 1, mem, &a.arcs_out));
    KMU_TRY(place_output(ctx, "cl.readsout", reads_out, n_reads, mem, &a.reads_out));
    KMU_HIP(ctx, hipMemsetAsync(zeros, 0, n_zero * 4, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.sole1, 0xFF, 2 * n_v * 4, ctx->stream));

    const dim3 per_arc(grid_for(ctx, n_arcs, 256)), per_v(grid_for(ctx, n_v, 256)), block(256);
    KMU_TRY(launch(ctx, "k_cl_check", k_cl_check, per_arc, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_tips", k_cl_tips, per_v, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_spare", k_cl_spare, per_v, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_tipkill", k_cl_tipkill, per_v, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_flag_tip", k_cl_flag, per_arc, block, 0, a, a.arcs, KMU_SG_ARC_TIP, a.deg2, a.sole2, (int) CL_ARCS_TIP, -1));
    KMU_TRY(launch(ctx, "k_cl_bubbles", k_cl_bubbles, per_v, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_flag_bubble", k_cl_flag, per_arc, block, 0, a, a.arcs_out, KMU_SG_ARC_BUBBLE, a.deg3, nullptr,
                   (int) CL_ARCS_BUBBLE, (int) CL_ARCS_LEFT));
    KMU_TRY(launch(ctx, "k_cl_unique", k_cl_unique, per_arc, block, 0, a));
    KMU_TRY(launch(ctx, "k_cl_reads", k_cl_reads, dim3(grid_for(ctx, n_reads, 256)), block, 0, a));

    // the stats and the refusal flag come to the host (the synchronisation)
    uint32_t h[18];
    KMU_TRY(read_back(ctx, {{h, zeros, sizeof h}}));
    if (h[16]) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED,
                    "`from` decreases, or a surviving arc names a vertex that does not exist, joins a read with itself, has no "
                    "surviving mate of its rec or touches a contained read");
    }
    static_assert(sizeof(kmu_sg_clean_stats) == 64, "8 counters");
    memcpy(stats_out, h, sizeof(kmu_sg_clean_stats));
    KMU_TRY(bring_output(ctx, arcs_out, a.arcs_out, n_arcs, mem));
    KMU_TRY(bring_output(ctx, reads_out, a.reads_out, n_reads, mem));
    return finish_call(ctx, mem);
}

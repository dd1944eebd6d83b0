// kmu_unitigs.hip -- from the unique arcs of the string graph to the unitigs: the ordered reads of every unitig with their
// coordinates, and the bases of every unitig, on the device (kmu_sg_unitigs, kmu_sg_unitig_seqs; the contract is in include/kmu.h,
// the arithmetic in kmu_ut_core.h; the walk from the items' ends to the output bytes is the segmented byte gather of kmu_gather.h).
//
//  k_ut_links      one lane per arc: a unique arc passes the range checks first (one that fails raises bad and is never used as an
//                  index), then integer atomic adds count the unique out-degree of `from` and in-degree of `to` -- a count above 1
//                  raises bad -- and next, prev and in are stored.
//  k_ut_mates      one lane per vertex: next[v] = w needs next[w ^ 1] = v ^ 1.
//  k_ut_init       one lane per vertex: the state of a segment of one vertex (kmu_ut_core.h) and its contribution.
//  k_ut_round      one lane per vertex: joins the segment of v with that of its ancestor.  Each round is a launch of its own that
//                  reads one buffer and writes the other, so nothing depends on timing and no workgroup waits on another.
//  k_ut_cut        one lane per vertex: the smallest vertex of a cycle loses its prev, the vertex before it its next; the in-degree
//                  stays, so the start still contributes the closing arc's length.  init and the rounds are then launched once more;
//                  where nothing was cut (a device flag) they return at once and the first ranking stands.
//  k_ut_tails      one lane per vertex: a vertex without next publishes its path's smallest vertex at the head and, if the path is
//                  kept, 1 and the number of reads at the smallest read.  Two device_scan_u32 over the reads give the numbering and
//                  `first`.
//  k_ut_write      one lane per vertex: the step and the place of a kept vertex, the unitig record by the tail.  It returns at once
//                  where bad is raised, so the outputs of a refused call stay untouched also in device memory.
//  k_ut_seq_lens   one lane per unitig: its slice of the step list is checked, its length and its number of steps go to the scans.
//  k_ut_seq_check  one lane per ITEM (unitig, step of it): the unitig by a binary search over the scanned step counts, the checks of
//                  the step against the one before it.  Unitigs may share steps, so the items, not the steps, are the work.
//  k_ut_seq_offs   one lane per unitig: the 64-bit offsets from the two 32-bit scans (k_gather_offsets under this timer name).
//  k_ut_seq_ends   one lane per item: the global end seq_offsets[u] + end of the item and its step.
//  k_ut_seq_copy   gather_tiles (kmu_gather.h) over the global ends: the byte of item r comes from its step's read; a reverse step
//                  reads backwards through the complement.
#include <algorithm>

#include "kmu_ut_core.h"
#include "kmu_gather.h"
#include "kmu_ctx.hpp"

namespace kmu {

struct UtArgs {
    const kmu_sg_arc *arcs;
    uint64_t n_arcs;
    const kmu_sg_read *reads; // or null
    const uint64_t *off;      // n_reads + 1
    uint32_t n_reads;
    uint32_t *next, *prev, *in, *outdeg, *indeg; // per vertex
    uint32_t *bad;                               // kernels only store 1 to it
    uint32_t *cut;                               // k_ut_cut stores 1 to it where it cuts a cycle
    uint32_t *pmin;                              // per vertex: at a head, the smallest vertex of its path
    uint32_t *keep, *size;                       // per read: at the smallest read of a kept path
    const uint64_t *uid, *firsts;                // their exclusive scans, n_reads + 1
    kmu_sg_unitig *unitigs;
    kmu_sg_step *path;
    kmu_sg_place *place; // or null
};

__device__ __forceinline__ uint64_t ut_read_len(const UtArgs &a, uint32_t r) { return a.off[r + 1] - a.off[r]; }
__device__ __forceinline__ bool ut_contained(const UtArgs &a, uint32_t r) { return a.reads && (a.reads[r].flags & KMU_SG_READ_CONTAINED); }

__global__ void __launch_bounds__(256) k_ut_links(UtArgs a) {
    bool bad = false;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_arcs; i += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_sg_arc x = a.arcs[i];
        if (x.unique != 1u) continue;
        bool ok = ut_arc_range_ok(x, a.n_reads);
        if (ok) {
            const uint32_t rf = x.from >> 1, rt = x.to >> 1;
            ok = ut_arc_reads_ok(x, ut_read_len(a, rt), a.reads ? a.reads[rf].flags : 0u, a.reads ? a.reads[rt].flags : 0u);
        }
        if (ok) {
            const uint32_t o = atomicAdd(&a.outdeg[x.from], 1u), n = atomicAdd(&a.indeg[x.to], 1u);
            ok = o == 0u && n == 0u;
            if (o == 0u) a.next[x.from] = x.to;
            if (n == 0u) {
                a.prev[x.to] = x.from;
                a.in[x.to] = x.len;
            }
        }
        bad |= !ok;
    }
    if (bad) *a.bad = 1u;
}

__global__ void __launch_bounds__(256) k_ut_mates(UtArgs a) {
    const uint64_t n_v = 2ull * a.n_reads;
    bool bad = false;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x)
        bad |= !ut_mate_ok(a.next, (uint32_t) v);
    if (bad) *a.bad = 1u;
}

// go: null in the first pass; in the second the flag of k_ut_cut -- where no cycle was cut the first ranking stands, and the second
// pass, launched all the same (the host does not know), returns at once and leaves both buffers as they are
__global__ void __launch_bounds__(256) k_ut_init(UtArgs a, UtState *s_out, uint64_t *d_out, const uint32_t *go) {
    if (go && !*go) return;
    const uint64_t n_v = 2ull * a.n_reads;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        s_out[v] = ut_state_init((uint32_t) v, a.prev[v]);
        d_out[v] = ut_contribution(a.indeg[v], a.in[v], ut_read_len(a, (uint32_t) (v >> 1)));
    }
}

__global__ void __launch_bounds__(256) k_ut_round(uint64_t n_v, const UtState *s_in, const uint64_t *d_in, UtState *s_out, uint64_t *d_out,
                                                  const uint32_t *go) {
    if (go && !*go) return;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t d;
        s_out[v] = ut_round(s_in, d_in, (uint32_t) v, d);
        d_out[v] = d;
    }
}

__global__ void __launch_bounds__(256) k_ut_cut(UtArgs a, const UtState *s_in) {
    const uint64_t n_v = 2ull * a.n_reads;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        if (!ut_cycle_start(s_in[v], (uint32_t) v)) continue;
        const uint32_t p = a.prev[v]; // (a vertex of a cycle has one; every stored link has passed the range checks)
        a.prev[v] = KMU_SG_NONE;
        if (p < n_v) a.next[p] = KMU_SG_NONE;
        *a.cut = 1u;
    }
}

__global__ void __launch_bounds__(256) k_ut_tails(UtArgs a, const UtState *s_in) {
    const uint64_t n_v = 2ull * a.n_reads;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        if (a.next[v] != KMU_SG_NONE) continue;
        const UtState s = s_in[v];
        if (s.top >= n_v || s.minv >= n_v) continue; // (never: both are vertices)
        a.pmin[s.top] = s.minv;
        if (ut_kept(s.minv) && !ut_contained(a, (uint32_t) (v >> 1))) {
            a.keep[s.minv >> 1] = 1u;
            a.size[s.minv >> 1] = s.cnt;
        }
    }
}

__global__ void __launch_bounds__(256) k_ut_write(UtArgs a, const UtState *s_in, const uint64_t *d_in) {
    if (*a.bad) return; // a refused call leaves its outputs untouched
    const uint64_t n_v = 2ull * a.n_reads;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t r = (uint32_t) (v >> 1), strand = (uint32_t) (v & 1u);
        if (ut_contained(a, r)) {
            if (!strand && a.place) a.place[r] = kmu_sg_place{KMU_SG_NONE, 0u, 0u, 0u};
            continue;
        }
        const UtState s = s_in[v];
        if (s.top >= n_v) continue; // (never)
        const uint32_t m = a.pmin[s.top];
        if (m >= n_v || !ut_kept(m)) continue;
        const uint32_t mr = m >> 1, rank = s.cnt - 1u;
        const uint64_t u = a.uid[mr], first = a.firsts[mr], at = first + rank, end = d_in[v];
        if (u >= a.n_reads || at >= a.n_reads) continue; // (never: both counts are <= n_reads)
        a.path[at] = kmu_sg_step{r, strand, end};
        if (a.place) a.place[r] = kmu_sg_place{(uint32_t) u, rank, strand, 0u};
        if (a.next[v] == KMU_SG_NONE) {
            const bool circular = a.indeg[s.top] == 1u && a.prev[s.top] == KMU_SG_NONE;
            a.unitigs[u] = kmu_sg_unitig{first, end, s.cnt, circular ? KMU_SG_UNITIG_CIRCULAR : 0u, mr, 0u};
        }
    }
}

// ---- kmu_sg_unitig_seqs ---------------------------------------------------------------------------------------------------------------
struct UsArgs {
    const kmu_sg_unitig *unitigs;
    uint64_t n_unitigs;
    const kmu_sg_step *path;
    uint64_t n_steps;
    const uint8_t *bases;
    const uint64_t *off; // n_reads + 1
    uint32_t n_reads;
    uint32_t *len_lo, *len_hi, *cnt, *bad;          // per unitig
    const uint64_t *off_lo, *off_hi, *item_off;     // their scans, n_unitigs + 1
    uint64_t *seq_off;                              // n_unitigs + 1
    uint64_t *ends;                                 // n_items + 1: ends[j + 1] is the global end of item j, ends[0] = 0
    uint64_t *isrc;                                 // n_items: the step of item j
    uint8_t *out;
    uint64_t total, n_items, n_tiles;
};

__global__ void __launch_bounds__(256) k_ut_seq_lens(UsArgs p) {
    bool bad = false;
    for (uint64_t u = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; u < p.n_unitigs; u += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_sg_unitig x = p.unitigs[u];
        const bool ok = ut_slice_ok(x, p.n_steps);
        bad |= !ok;
        p.len_lo[u] = ok ? (uint32_t) x.len : 0u;
        p.len_hi[u] = ok ? (uint32_t) (x.len >> 32) : 0u;
        p.cnt[u] = ok ? x.n_reads : 0u;
    }
    if (bad) *p.bad = 1u;
}

// item j: its unitig and its step; false beyond the last item
__device__ __forceinline__ bool ut_item(const UsArgs &p, uint64_t j, uint64_t &u, uint64_t &i) {
    if (j >= p.item_off[p.n_unitigs]) return false;
    u = gather_upper_index(p.item_off, p.n_unitigs, j); // (item_off[u] <= j < item_off[n_unitigs]: u < n_unitigs, and u is not empty)
    i = j - p.item_off[u];
    return u < p.n_unitigs;
}

__global__ void __launch_bounds__(256) k_ut_seq_check(UsArgs p) {
    bool bad = false;
    const uint64_t n_items = p.item_off[p.n_unitigs];
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < n_items; j += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t u, i;
        if (!ut_item(p, j, u, i)) continue;
        const kmu_sg_unitig x = p.unitigs[u];
        const uint64_t at = x.first + i;
        if (at >= p.n_steps) continue; // (never: k_ut_seq_lens gave a bad slice no items)
        const kmu_sg_step s = p.path[at];
        const uint64_t prev_end = i ? p.path[at - 1u].end : 0ull;
        const uint64_t read_len = s.read < p.n_reads ? p.off[s.read + 1u] - p.off[s.read] : 0ull;
        bad |= !ut_step_ok(s, p.n_reads, prev_end, read_len, i + 1u == x.n_reads, x.len);
    }
    if (bad) *p.bad = 1u;
}

__global__ void __launch_bounds__(256) k_ut_seq_ends(UsArgs p) {
    for (uint64_t j = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; j < p.n_items; j += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t u, i;
        if (j == 0) p.ends[0] = 0ull;
        if (!ut_item(p, j, u, i)) continue;
        const uint64_t at = p.unitigs[u].first + i;
        p.isrc[j] = at;
        p.ends[j + 1u] = p.seq_off[u] + (at < p.n_steps ? p.path[at].end : 0ull);
    }
}

__global__ void __launch_bounds__(256) k_ut_seq_copy(UsArgs p) {
    gather_tiles(p.ends, p.n_items, p.total, p.n_tiles, [&](uint64_t r, uint64_t o) {
        if (r >= p.n_items) return; // (never)
        const uint64_t begin = p.ends[r], at = p.isrc[r];
        const kmu_sg_step s = p.path[at < p.n_steps ? at : 0u];
        if (s.read >= p.n_reads) return; // (k_ut_seq_check has checked the steps: never)
        const uint64_t b0 = p.off[s.read], len = p.off[s.read + 1u] - b0;
        const uint64_t idx = ut_src_index(s.strand, len, p.ends[r + 1u] - begin, o - begin);
        if (idx < len) {
            const uint8_t b = p.bases[b0 + idx];
            p.out[o] = s.strand ? ut_complement(b) : b;
        }
    });
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_sg_unitigs(kmu_ctx *ctx, const kmu_sg_arc *arcs, uint64_t n_arcs, const kmu_sg_read *reads, const uint64_t *offsets,
                              uint32_t n_reads, int mem, kmu_sg_unitig *unitigs_out, kmu_sg_step *path_out, kmu_sg_place *place_out,
                              uint64_t *n_steps_out, uint64_t *n_out) {
    if (!ctx || !offsets || !n_out || !unitigs_out || !path_out || (!arcs && n_arcs)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    KMU_TRY(check_mem(ctx, mem));
    if (n_reads >= 0x80000000u) return fail(ctx, KMU_E_UNSUPPORTED, "%u reads: 2^31 or more", n_reads);
    if (n_reads == 0) {
        if (n_arcs) return fail(ctx, KMU_E_BAD_ARG, "arcs but no reads");
        *n_out = 0;
        if (n_steps_out) *n_steps_out = 0;
        return KMU_OK;
    }
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    UtArgs a{};
    KMU_TRY(stage_to_device(ctx, "ut.arcs", arcs, (size_t) n_arcs, mem, &a.arcs));
    a.n_arcs = n_arcs;
    KMU_TRY(stage_to_device(ctx, "ut.reads", reads, (size_t) n_reads, mem, &a.reads));
    KMU_TRY(stage_to_device(ctx, "ut.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;

    // the workspace: links (next and prev start as KMU_SG_NONE), degrees and per-read counts (start as 0), states
    const size_t n_v = 2 * (size_t) n_reads;
    uint32_t *links, *zeros;
    KMU_TRY(dev_array(ctx, "ut.links", 2 * n_v, &links));
    KMU_TRY(dev_array(ctx, "ut.zeros", 2 * n_v + 2 * (size_t) n_reads + 2, &zeros));
    KMU_TRY(dev_array(ctx, "ut.in", n_v, &a.in));
    KMU_TRY(dev_array(ctx, "ut.pmin", n_v, &a.pmin));
    a.next = links;
    a.prev = links + n_v;
    a.outdeg = zeros;
    a.indeg = zeros + n_v;
    a.keep = zeros + 2 * n_v;
    a.size = a.keep + n_reads;
    a.bad = a.size + n_reads;
    a.cut = a.bad + 1;
    UtState *st[2];
    uint64_t *dist[2], *uid, *firsts;
    KMU_TRY(dev_array(ctx, "ut.s0", n_v, &st[0]));
    KMU_TRY(dev_array(ctx, "ut.s1", n_v, &st[1]));
    KMU_TRY(dev_array(ctx, "ut.d0", n_v, &dist[0]));
    KMU_TRY(dev_array(ctx, "ut.d1", n_v, &dist[1]));
    KMU_TRY(dev_array(ctx, "ut.uid", (size_t) n_reads + 1, &uid));
    KMU_TRY(dev_array(ctx, "ut.firsts", (size_t) n_reads + 1, &firsts));
    a.uid = uid;
    a.firsts = firsts;
    KMU_TRY(place_output(ctx, "ut.unitigs", unitigs_out, n_reads, mem, &a.unitigs));
    KMU_TRY(place_output(ctx, "ut.path", path_out, n_reads, mem, &a.path));
    KMU_TRY(place_output(ctx, "ut.place", place_out, n_reads, mem, &a.place));
    KMU_HIP(ctx, hipMemsetAsync(links, 0xFF, 2 * n_v * 4, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(zeros, 0, (2 * n_v + 2 * (size_t) n_reads + 2) * 4, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.pmin, 0xFF, n_v * 4, ctx->stream));

    const dim3 per_v(grid_for(ctx, n_v, 256)), block(256);
    const uint32_t rounds = ut_rounds(n_v);
    KMU_TRY(launch(ctx, "k_ut_links", k_ut_links, dim3(grid_for(ctx, n_arcs, 256)), block, 0, a));
    KMU_TRY(launch(ctx, "k_ut_mates", k_ut_mates, per_v, block, 0, a));
    int cur = 0;
    for (int pass = 0; pass < 2; pass++) { // pass 0 ranks the paths and finds the cycles, pass 1 ranks again where a cycle was cut
        const uint32_t *go = pass ? a.cut : nullptr;
        cur = 0; // (both passes end in the same buffer, so a second pass that returns at once leaves the first one's result there)
        KMU_TRY(launch(ctx, "k_ut_init", k_ut_init, per_v, block, 0, a, st[0], dist[0], go));
        for (uint32_t r = 0; r < rounds; r++, cur ^= 1)
            KMU_TRY(launch(ctx, "k_ut_round", k_ut_round, per_v, block, 0, (uint64_t) n_v, st[cur], dist[cur], st[cur ^ 1], dist[cur ^ 1], go));
        if (pass == 0) KMU_TRY(launch(ctx, "k_ut_cut", k_ut_cut, per_v, block, 0, a, st[cur]));
    }
    KMU_TRY(launch(ctx, "k_ut_tails", k_ut_tails, per_v, block, 0, a, st[cur]));
    KMU_TRY(device_scan_u32(ctx, a.keep, n_reads, uid));
    KMU_TRY(device_scan_u32(ctx, a.size, n_reads, firsts));
    KMU_TRY(launch(ctx, "k_ut_write", k_ut_write, per_v, block, 0, a, st[cur], dist[cur]));

    // the two counts and the refusal flag come to the host (the synchronisation)
    uint32_t h_bad = 0;
    uint64_t n_unitigs = 0, n_steps = 0;
    KMU_TRY(read_back(ctx, {{&h_bad, a.bad}, {&n_unitigs, uid + n_reads}, {&n_steps, firsts + n_reads}}));
    if (h_bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED,
                    "a unique arc names a vertex that does not exist, joins a read with itself, is longer than its read, is reduced, "
                    "touches a contained read, shares a vertex with another unique arc or has no mate");
    }
    *n_out = n_unitigs;
    if (n_steps_out) *n_steps_out = n_steps;
    KMU_TRY(bring_output(ctx, unitigs_out, a.unitigs, n_unitigs, mem));
    KMU_TRY(bring_output(ctx, path_out, a.path, n_steps, mem));
    KMU_TRY(bring_output(ctx, place_out, a.place, n_reads, mem));
    return finish_call(ctx, mem);
}

extern "C" int kmu_sg_unitig_seqs(kmu_ctx *ctx, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path, uint64_t n_steps,
                                  const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int mem, uint64_t *seq_offsets_out,
                                  uint8_t *seq_out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !offsets || !n_out || (!unitigs && n_unitigs) || (!path && n_steps)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    KMU_TRY(check_mem(ctx, mem));
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_unitigs == 0) {
        if (seq_out) KMU_TRY(zero_first_offset(ctx, seq_offsets_out, mem));
        return finish_call(ctx, mem);
    }
    UsArgs a{};
    KMU_TRY(stage_to_device(ctx, "us.unitigs", unitigs, (size_t) n_unitigs, mem, &a.unitigs));
    a.n_unitigs = n_unitigs;
    KMU_TRY(stage_to_device(ctx, "us.path", path, (size_t) n_steps, mem, &a.path));
    a.n_steps = n_steps;
    KMU_TRY(stage_to_device(ctx, "us.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;
    uint64_t *off_lo, *off_hi, *item_off;
    KMU_TRY(dev_array(ctx, "us.lenlo", n_unitigs, &a.len_lo));
    KMU_TRY(dev_array(ctx, "us.lenhi", n_unitigs, &a.len_hi));
    KMU_TRY(dev_array(ctx, "us.cnt", n_unitigs, &a.cnt));
    KMU_TRY(dev_array(ctx, "us.offlo", n_unitigs + 1, &off_lo));
    KMU_TRY(dev_array(ctx, "us.offhi", n_unitigs + 1, &off_hi));
    KMU_TRY(dev_array(ctx, "us.itemoff", n_unitigs + 1, &item_off));
    KMU_TRY(dev_array(ctx, "us.bad", 1, &a.bad));
    a.off_lo = off_lo;
    a.off_hi = off_hi;
    a.item_off = item_off;
    KMU_HIP(ctx, hipMemsetAsync(a.bad, 0, 4, ctx->stream));

    // the checks, the lengths and the item counts; the refusal comes before any output (synchronisation)
    const dim3 per_u(grid_for(ctx, n_unitigs + 1, 256)), block(256);
    KMU_TRY(launch(ctx, "k_ut_seq_lens", k_ut_seq_lens, per_u, block, 0, a));
    KMU_TRY(device_scan_u32(ctx, a.len_lo, n_unitigs, off_lo));
    KMU_TRY(device_scan_u32(ctx, a.len_hi, n_unitigs, off_hi));
    KMU_TRY(device_scan_u32(ctx, a.cnt, n_unitigs, item_off));
    KMU_TRY(launch(ctx, "k_ut_seq_check", k_ut_seq_check, dim3(grid_for(ctx, std::max(n_steps, n_unitigs), 256)), block, 0, a));
    uint32_t h_bad = 0;
    uint64_t t_lo = 0, t_hi = 0;
    KMU_TRY(read_back(ctx, {{&h_bad, a.bad}, {&t_lo, off_lo + n_unitigs}, {&t_hi, off_hi + n_unitigs}, {&a.n_items, item_off + n_unitigs}}));
    if (h_bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED,
                    "a unitig's steps lie outside the step list, a step names a read that does not exist or a strand above 1, ends "
                    "decrease, a contribution is above the length of its read, or the last end is not the unitig's len");
    }
    a.total = t_lo + (t_hi << 32);
    *n_out = a.total;
    if (!seq_out) return finish_call(ctx, mem);
    if (cap < a.total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "cap = %llu is below the %llu bytes", (unsigned long long) cap, (unsigned long long) a.total);
    }
    if (!bases && a.total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "null argument");
    }
    a.seq_off = seq_offsets_out;
    if (mem == KMU_MEM_HOST || !seq_offsets_out) KMU_TRY(dev_array(ctx, "us.seqoff", n_unitigs + 1, &a.seq_off));
    KMU_TRY(launch(ctx, "k_ut_seq_offs", k_gather_offsets, per_u, block, 0, a.off_lo, a.off_hi, n_unitigs, a.seq_off));
    KMU_TRY(bring_output(ctx, seq_offsets_out, a.seq_off, n_unitigs + 1, mem));
    if (a.total) {
        // (the batch's size is its last offset)
        KMU_TRY(stage_to_device(ctx, "us.bases", bases, mem == KMU_MEM_HOST ? (size_t) offsets[n_reads] : 0, mem, &a.bases));
        KMU_TRY(dev_array(ctx, "us.ends", (size_t) a.n_items + 1, &a.ends));
        KMU_TRY(dev_array(ctx, "us.isrc", (size_t) a.n_items, &a.isrc));
        a.n_tiles = (a.total + GATHER_TILE - 1u) / GATHER_TILE;
        KMU_TRY(place_output(ctx, "us.out", seq_out, (size_t) a.total, mem, &a.out));
        KMU_TRY(launch(ctx, "k_ut_seq_ends", k_ut_seq_ends, dim3(grid_for(ctx, a.n_items, 256)), block, 0, a));
        KMU_TRY(launch(ctx, "k_ut_seq_copy", k_ut_seq_copy, dim3(grid_for(ctx, a.n_tiles, 4)), block, 0, a));
        KMU_TRY(bring_output(ctx, seq_out, a.out, (size_t) a.total, mem));
    }
    return finish_call(ctx, mem);
}

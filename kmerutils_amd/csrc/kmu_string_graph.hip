// kmu_string_graph.hip -- from the chain records of a self-join to the string graph: the class of every record, the contained
// reads, the bidirected overlap graph of the dovetails and its transitive reduction, on the device (kmu_sg_classify, kmu_sg_graph;
// the contract is in include/kmu.h, the arithmetic in kmu_sg_core.h).
//
//  k_sg_classify  one lane per record: the range checks (a record that fails one raises bad, gets class 0 and is never used as an
//                 index; the call is refused at its synchronisation), the class, an atomic OR of the contained flag and integer
//                 atomic adds of the record counts -- they commute, so the summaries are a pure function of the records.
//  k_sg_arcs      COUNT and WRITE.  One wave per tile of KMU_SG_TILE records, one lane per record: a DOVETAIL whose two reads are
//                 both not contained survives, survivors are compacted in record order by ballot and prefix count.  COUNT leaves one
//                 count per tile and device_scan_u32 the offsets; WRITE leaves survivor q's two sort entries, key from << 32 | to,
//                 value 2c + side, at 2q and 2q + 1: the entries are in arc-id order, so the stable sort ends in (from, to, rec).
//  sort           radix_sort_pairs_passes over the bytes 2 n_reads can reach.
//  k_sg_fill      one lane per sorted entry: the arc record, recomputed from the chain record (40 bytes read against 24 more bytes
//                 per entry carried through the sort).
//  k_sg_heads     one lane per vertex: two binary searches give its slice (arc_offsets), one walk over the slice L(v) - fuzz and
//                 first(v).
//  k_sg_reduce    the hot kernel.  One wave per arc f = v -> w, arcs dealt grid-stride, so a repeat vertex of degree d is spread over
//                 d waves.  The lanes stride over out(w); a lane tests the rule for its g = w -> x, binary-searches the run of
//                 to == x in out(v) and stores 1 to mark[rec] for every arc of the run: identical idempotent byte stores, no atomics.
//  k_sg_finish    one lane per arc: KMU_SG_ARC_REDUCED from mark[rec] (the mate has the same rec), otherwise an integer atomic add
//                 to the surviving out-degree of `from`.
//  k_sg_unique    one lane per arc: an arc that survives is in out(from) and its mate in out(to ^ 1), so it is unique iff both
//                 surviving degrees are 1 -- two loads instead of a search for the mate.
#include <algorithm>

#include "kmu_sg_core.h"
#include "kmu_sort.h"

namespace kmu {

static_assert(KMU_SG_TILE % 64 == 0, "a tile is walked in chunks of one wave");

struct SgArgs {
    const kmu_chain *chains;
    const kmu_chain_aln *aln; // or null
    const uint64_t *off;      // n_reads + 1
    uint64_t n_chains;
    uint32_t n_reads;
    kmu_sg_params p;
    uint8_t *cls;       // per record
    kmu_sg_read *reads; // per read
    uint32_t *bad;      // kernels only OR into it
    uint32_t n_tiles;
    uint32_t *counts;     // survivors per tile
    const uint64_t *coff; // their exclusive scan
    uint64_t n_arcs;
    uint64_t *keys; // sort entries
    uint32_t *vals;
    kmu_sg_arc *arcs;  // sorted
    uint64_t *arc_off; // 2 n_reads + 1
    uint32_t *max_len; // per vertex
    uint32_t *first;   // per vertex: the index of first(v)
    uint8_t *mark;     // per record
};

__device__ __forceinline__ uint64_t sg_read_len(const SgArgs &a, uint32_t r) { return a.off[r + 1] - a.off[r]; }

__global__ void __launch_bounds__(256) k_sg_classify(SgArgs a) {
    uint32_t bad = 0;
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c < a.n_chains; c += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_chain r = a.chains[c];
        uint32_t cls = KMU_SG_SKIP;
        bool ok = sg_record_ok(r, a.n_reads);
        uint64_t la = 0, lb = 0;
        if (ok) {
            la = sg_read_len(a, r.read_a);
            lb = sg_read_len(a, r.read_b);
            ok = sg_lengths_ok(r, la, lb);
        }
        if (!ok) {
            bad = 1;
        } else {
            cls = sg_class(r, la, lb, a.aln ? a.aln + c : nullptr, a.p);
            if (cls != KMU_SG_SKIP) {
                atomicAdd(&a.reads[r.read_a].n_records, 1u);
                atomicAdd(&a.reads[r.read_b].n_records, 1u);
            }
            if (cls == KMU_SG_A_CONTAINED) atomicOr(&a.reads[r.read_a].flags, KMU_SG_READ_CONTAINED);
            if (cls == KMU_SG_B_CONTAINED) atomicOr(&a.reads[r.read_b].flags, KMU_SG_READ_CONTAINED);
        }
        a.cls[c] = (uint8_t) cls;
    }
    if (bad) atomicOr(a.bad, 1u);
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_sg_arcs(SgArgs a) {
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t t0 = (uint64_t) tile * KMU_SG_TILE;
    uint64_t at = WRITE ? a.coff[tile] : 0ull;
    for (uint32_t c0 = 0; c0 < KMU_SG_TILE; c0 += 64) { // uniform trip count: all lanes reach the ballot
        const uint64_t c = t0 + c0 + lane;
        bool pass = false;
        kmu_chain r{};
        if (c < a.n_chains && a.cls[c] == KMU_SG_DOVETAIL) { // (a DOVETAIL has passed the range checks)
            r = a.chains[c];
            pass = !((a.reads[r.read_a].flags | a.reads[r.read_b].flags) & KMU_SG_READ_CONTAINED);
        }
        const uint64_t bal = __ballot(pass);
        if (WRITE) {
            const uint64_t q = at + (uint64_t) __popcll(bal & below);
            if (pass && 2u * q + 1u < a.n_arcs) {
                kmu_sg_arc x, y;
                sg_arc_pair(r, sg_read_len(a, r.read_a), sg_read_len(a, r.read_b), (uint32_t) c, x, y);
                a.keys[2u * q] = sg_arc_key(x);
                a.vals[2u * q] = 2u * (uint32_t) c;
                a.keys[2u * q + 1u] = sg_arc_key(y);
                a.vals[2u * q + 1u] = 2u * (uint32_t) c + 1u;
            }
        }
        at += (uint64_t) __popcll(bal);
    }
    if (!WRITE && lane == 0) a.counts[tile] = (uint32_t) at;
}

__global__ void __launch_bounds__(256) k_sg_fill(SgArgs a) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_arcs; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t id = a.vals[i], c = id >> 1;
        kmu_sg_arc x{}, y{};
        if (c < a.n_chains) { // (always: the ids are the ones k_sg_arcs wrote)
            const kmu_chain r = a.chains[c];
            sg_arc_pair(r, sg_read_len(a, r.read_a), sg_read_len(a, r.read_b), c, x, y);
        }
        const bool b_side = id & 1u; // (field by field: a select between the two structs goes through scratch)
        kmu_sg_arc o;
        o.from = b_side ? y.from : x.from;
        o.to = b_side ? y.to : x.to;
        o.len = b_side ? y.len : x.len;
        o.ovl = b_side ? y.ovl : x.ovl;
        o.rec = c;
        o.flags = o.unique = o.zero = 0u;
        a.arcs[i] = o;
    }
}

__global__ void __launch_bounds__(256) k_sg_heads(SgArgs a) {
    const uint64_t n_v = 2ull * a.n_reads;
    for (uint64_t v = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; v < n_v; v += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t lo = sg_lower_from(a.arcs, a.n_arcs, v), hi = sg_lower_from(a.arcs, a.n_arcs, v + 1u);
        uint32_t max_len;
        uint64_t first;
        sg_vertex_stats(a.arcs, lo, hi, max_len, first);
        a.arc_off[v] = lo;
        a.max_len[v] = max_len;
        a.first[v] = (uint32_t) first;
        if (v + 1u == n_v) a.arc_off[n_v] = a.n_arcs;
    }
}

__global__ void __launch_bounds__(256) k_sg_reduce(SgArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t waves = (uint64_t) gridDim.x * (blockDim.x / 64u), n_v = 2ull * a.n_reads;
    uint8_t *mark = a.mark;
    const uint64_t n_chains = a.n_chains;
    for (uint64_t f = (uint64_t) blockIdx.x * (blockDim.x / 64u) + threadIdx.x / 64u; f < a.n_arcs; f += waves) {
        const uint32_t v = a.arcs[f].from, w = a.arcs[f].to, len_f = a.arcs[f].len; // wave-uniform
        if (v >= n_v || w >= n_v) continue;                                          // (never: k_sg_fill wrote them)
        const uint64_t v_lo = a.arc_off[v], v_hi = a.arc_off[v + 1], w_lo = a.arc_off[w], w_hi = a.arc_off[w + 1];
        const uint32_t max_len_v = a.max_len[v];
        const uint64_t first_w = a.first[w];
        for (uint64_t j = w_lo + lane; j < w_hi; j += 64)
            sg_reduce_step(a.arcs, len_f, v_lo, v_hi, max_len_v, j, first_w, a.p.fuzz, [mark, n_chains](uint32_t rec) {
                if (rec < n_chains) mark[rec] = 1;
            });
    }
}

__device__ __forceinline__ uint32_t *sg_degree(const SgArgs &a, uint32_t v) {
    kmu_sg_read *r = a.reads + (v >> 1);
    return (v & 1u) ? &r->out_rev : &r->out_fwd;
}

__global__ void __launch_bounds__(256) k_sg_finish(SgArgs a) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_arcs; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t rec = a.arcs[i].rec, from = a.arcs[i].from;
        if (rec >= a.n_chains || (from >> 1) >= a.n_reads) continue; // (never)
        if (a.mark[rec]) a.arcs[i].flags = KMU_SG_ARC_REDUCED;
        else atomicAdd(sg_degree(a, from), 1u);
    }
}

__global__ void __launch_bounds__(256) k_sg_unique(SgArgs a) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_arcs; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t from = a.arcs[i].from, to = a.arcs[i].to;
        if ((from >> 1) >= a.n_reads || (to >> 1) >= a.n_reads || a.arcs[i].flags) continue;
        if (*sg_degree(a, from) == 1u && *sg_degree(a, to ^ 1u) == 1u) a.arcs[i].unique = 1u;
    }
}

} // namespace kmu

using namespace kmu;

static const char *const SG_REFUSAL =
    "a record names a read that does not exist, a strand above 1, a start above its end, an end above the length of its read, or a "
    "read of 2^32 bases or more";

// what both entry points refuse before anything is launched
static int sg_check(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const uint64_t *offsets, uint32_t n_reads,
                    const kmu_sg_params *p, int mem) {
    if (!ctx || !offsets || !p || (!chains && n_chains)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    if (p->int_permille > 1000u) return fail(ctx, KMU_E_BAD_ARG, "int_permille = %u: at most 1000", p->int_permille);
    if (p->min_identity_permille > 1000u) return fail(ctx, KMU_E_BAD_ARG, "min_identity_permille = %u: at most 1000", p->min_identity_permille);
    KMU_TRY(check_mem(ctx, mem));
    if (n_reads >= 0x80000000u) return fail(ctx, KMU_E_UNSUPPORTED, "%u reads: 2^31 or more", n_reads);
    if (n_chains >= 0x80000000ull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu records: 2^31 or more", (unsigned long long) n_chains);
    if (n_chains && !n_reads) return fail(ctx, KMU_E_BAD_ARG, "records but no reads");
    return KMU_OK;
}

// the inputs on the device, the classes and the summaries in the workspace, k_sg_classify enqueued
static int sg_begin(kmu_ctx *ctx, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains, const uint64_t *offsets,
                    uint32_t n_reads, const kmu_sg_params *p, int mem, SgArgs &a) {
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KMU_TRY(stage_to_device(ctx, "sg.chains", chains, (size_t) n_chains, mem, &a.chains));
    KMU_TRY(stage_to_device(ctx, "sg.aln", aln, (size_t) n_chains, mem, &a.aln));
    KMU_TRY(stage_to_device(ctx, "sg.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_chains = n_chains;
    a.n_reads = n_reads;
    a.p = *p;
    KMU_TRY(dev_array(ctx, "sg.cls", n_chains ? n_chains : 1, &a.cls));
    KMU_TRY(dev_array(ctx, "sg.reads", n_reads ? n_reads : 1, &a.reads));
    KMU_TRY(dev_array(ctx, "sg.bad", 1, &a.bad));
    KMU_HIP(ctx, hipMemsetAsync(a.reads, 0, (size_t) (n_reads ? n_reads : 1) * sizeof(kmu_sg_read), ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.bad, 0, 4, ctx->stream));
    return launch(ctx, "k_sg_classify", k_sg_classify, dim3(grid_for(ctx, n_chains, 256)), dim3(256), 0, a);
}

extern "C" int kmu_sg_classify(kmu_ctx *ctx, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains, const uint64_t *offsets,
                               uint32_t n_reads, const kmu_sg_params *p, int mem, uint8_t *class_out, kmu_sg_read *reads_out) {
    KMU_TRY(sg_check(ctx, chains, n_chains, offsets, n_reads, p, mem));
    if (!class_out || !reads_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    SgArgs a{};
    KMU_TRY(sg_begin(ctx, chains, aln, n_chains, offsets, n_reads, p, mem, a));
    uint32_t h_bad = 0;
    KMU_TRY(read_back(ctx, {{&h_bad, a.bad}}));
    if (h_bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED, "%s", SG_REFUSAL);
    }
    KMU_TRY(copy_out(ctx, class_out, a.cls, (size_t) n_chains, mem));
    KMU_TRY(copy_out(ctx, reads_out, a.reads, (size_t) n_reads * sizeof(kmu_sg_read), mem));
    return finish_call(ctx, mem);
}

extern "C" int kmu_sg_graph(kmu_ctx *ctx, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains, const uint64_t *offsets,
                            uint32_t n_reads, const kmu_sg_params *p, int mem, uint8_t *class_out, kmu_sg_read *reads_out,
                            kmu_sg_arc *arcs_out, uint64_t cap, uint64_t *arc_offsets_out, uint64_t *n_out) {
    KMU_TRY(sg_check(ctx, chains, n_chains, offsets, n_reads, p, mem));
    if (!n_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    SgArgs a{};
    KMU_TRY(sg_begin(ctx, chains, aln, n_chains, offsets, n_reads, p, mem, a));

    // the surviving dovetails: COUNT, the offsets; the total and the refusal flags come to the host (the synchronisation)
    a.n_tiles = (uint32_t) std::max<uint64_t>(1, (n_chains + KMU_SG_TILE - 1) / KMU_SG_TILE);
    uint64_t *coff;
    KMU_TRY(dev_array(ctx, "sg.counts", a.n_tiles, &a.counts));
    KMU_TRY(dev_array(ctx, "sg.coff", (size_t) a.n_tiles + 1, &coff));
    a.coff = coff;
    KMU_TRY(launch(ctx, "k_sg_arcs_count", k_sg_arcs<false>, dim3(a.n_tiles), dim3(64), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.counts, a.n_tiles, coff));
    uint32_t h_bad = 0;
    uint64_t survivors = 0;
    KMU_TRY(read_back(ctx, {{&h_bad, a.bad}, {&survivors, coff + a.n_tiles}}));
    if (h_bad) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED, "%s", SG_REFUSAL);
    }
    a.n_arcs = 2 * survivors; // (survivors <= n_chains < 2^31)
    *n_out = a.n_arcs;
    if (!arcs_out) return finish_call(ctx, mem);
    if (cap < a.n_arcs) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu arcs, room for %llu", (unsigned long long) a.n_arcs, (unsigned long long) cap);
    }

    const size_t n_v = 2 * (size_t) n_reads;
    KMU_TRY(dev_array(ctx, "sg.arcoff", n_v + 1, &a.arc_off));
    if (a.n_arcs == 0) {
        KMU_HIP(ctx, hipMemsetAsync(a.arc_off, 0, (n_v + 1) * 8, ctx->stream));
    } else {
        uint64_t *keys1;
        uint32_t *vals1;
        KMU_TRY(dev_array(ctx, "sg.keys0", a.n_arcs, &a.keys));
        KMU_TRY(dev_array(ctx, "sg.vals0", a.n_arcs, &a.vals));
        KMU_TRY(dev_array(ctx, "sg.keys1", a.n_arcs, &keys1));
        KMU_TRY(dev_array(ctx, "sg.vals1", a.n_arcs, &vals1));
        KMU_TRY(dev_array(ctx, "sg.maxlen", n_v, &a.max_len));
        KMU_TRY(dev_array(ctx, "sg.first", n_v, &a.first));
        KMU_TRY(dev_array(ctx, "sg.mark", n_chains, &a.mark));
        KMU_TRY(place_output(ctx, "sg.arcs", arcs_out, a.n_arcs, mem, &a.arcs));
        KMU_HIP(ctx, hipMemsetAsync(a.mark, 0, n_chains, ctx->stream));

        KMU_TRY(launch(ctx, "k_sg_arcs_write", k_sg_arcs<true>, dim3(a.n_tiles), dim3(64), 0, a));
        const uint32_t id_passes = radix_id_passes(2u * n_reads);
        KMU_TRY(radix_sort_pairs_passes(ctx, a.keys, a.vals, keys1, vals1, a.n_arcs, id_passes | (id_passes << 4), nullptr));
        const dim3 flat(grid_for(ctx, a.n_arcs, 256));
        KMU_TRY(launch(ctx, "k_sg_fill", k_sg_fill, flat, dim3(256), 0, a));
        KMU_TRY(launch(ctx, "k_sg_heads", k_sg_heads, dim3(grid_for(ctx, n_v, 256)), dim3(256), 0, a));
        KMU_TRY(launch(ctx, "k_sg_reduce", k_sg_reduce, dim3(grid_for(ctx, a.n_arcs, 4)), dim3(256), 0, a)); // (a wave per arc)
        KMU_TRY(launch(ctx, "k_sg_finish", k_sg_finish, flat, dim3(256), 0, a));
        KMU_TRY(launch(ctx, "k_sg_unique", k_sg_unique, flat, dim3(256), 0, a));
        KMU_TRY(bring_output(ctx, arcs_out, a.arcs, a.n_arcs, mem));
    }
    KMU_TRY(copy_out(ctx, class_out, a.cls, (size_t) n_chains, mem));
    KMU_TRY(copy_out(ctx, reads_out, a.reads, (size_t) n_reads * sizeof(kmu_sg_read), mem));
    KMU_TRY(copy_out(ctx, arc_offsets_out, a.arc_off, (n_v + 1) * 8, mem));
    return finish_call(ctx, mem);
}

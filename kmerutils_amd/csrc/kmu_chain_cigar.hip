// kmu_chain_cigar.hip -- for every chain record the alignment of kmu_chain_align AND its path as CIGAR runs, on the device
// (kmu_chain_cigar; the contract is in include/kmu.h, the direction bits, their layout and the walk in kmu_align_core.h, the sweep
// in kmu_align_sweep.h).
//
//  k_cigar_plan   one lane per chain: checks the record as k_chain_align does (a record that fails raises info[0]; the call is
//                 refused at the plan's synchronisation, before any sweep) and leaves the rows of the chain's trace slab -- 0 for a
//                 chain without DONE and for one whose slab alone is above the budget.  device_scan_u32 turns the rows into
//                 offsets; the host reads them and cuts the chains, in order, into batches whose slabs fit the budget together.
//  per batch:
//  k_cigar_sweep  k_chain_align on the chains of the batch, through the same align_chain; a chain with a slab runs the TRACE
//                 instance: per pair-step a lane ORs its 4 C direction bits into a word and stores the word when it is full
//                 (row r of the slab: 64 words, one coalesced 256-byte store of the wave).  Fire-and-forget: nothing waits for them.
//  k_cigar_walk   one wave per chain: walks the path back from (m, n).  The wave stages ALIGN_WALK_ROWS rows of the slab at a time
//                 in LDS (coalesced loads; the walk only ever moves towards lower rows) and every lane walks the same path inside
//                 the block -- the state is uniform, the LDS reads are broadcasts -- so a path step costs an LDS read, not a
//                 dependent global load.  Lane 0 writes the runs downwards from the END of the chain's own slab: they come out
//                 last-first, so ascending memory holds them in path order.  The rows they overwrite are staged or done with: a
//                 pair-step has at most two cells on the path (8 bytes of runs) and 32 C bytes of slab.
//  k_ing_scan     device_scan_u32 over the batch's run counts.
//  k_cigar_copy   one wave per chain: the runs from the end of the slab to ops_out + op_offsets[c], never beyond cap; the running
//                 total passes from batch to batch in device memory, so the call synchronises twice whatever the batches are.
#include "kmu_align_sweep.h"

namespace kmu {

static_assert(((ALIGN_DIR_OPS >> (4 * ALIGN_DIR_EQ)) & 15u) == KMU_CIGAR_EQ && ((ALIGN_DIR_OPS >> (4 * ALIGN_DIR_X)) & 15u) == KMU_CIGAR_X &&
                  ((ALIGN_DIR_OPS >> (4 * ALIGN_DIR_UP)) & 15u) == KMU_CIGAR_I && ((ALIGN_DIR_OPS >> (4 * ALIGN_DIR_LEFT)) & 15u) == KMU_CIGAR_D,
              "the header's codes are those of kmu_align_core.h");
static_assert(ALIGN_MAX_RUN == KMU_CIGAR_MAX_RUN, "the header names the longest run of kmu_align_core.h");

struct CigarArgs {
    AlignArgs a;
    uint64_t b0, b1;      // the chains of the batch
    const uint64_t *roff; // [n_chains + 1]: the rows of all slabs before a chain's; the batch's trace begins at row roff[b0]
    uint32_t *trace;
    uint32_t *cnt;        // [n_chains]: runs per chain
    uint64_t budget_rows; // (plan)
    uint32_t *rows;       // (plan) [n_chains]
};

// the checks of k_chain_align; beg_*: where the two reads begin
__device__ __forceinline__ bool cigar_record_ok(const AlignArgs &a, const kmu_chain &rec, uint64_t &beg_a, uint64_t &beg_b) {
    bool ok = rec.read_a < a.n_reads_q && rec.read_b < a.n_reads_db && rec.strand <= 1u && rec.a_start <= rec.a_end &&
              rec.b_start <= rec.b_end;
    beg_a = beg_b = 0;
    if (ok) {
        beg_a = a.off_q[rec.read_a];
        beg_b = a.off_db[rec.read_b];
        ok = rec.a_end <= a.off_q[rec.read_a + 1u] - beg_a && rec.b_end <= a.off_db[rec.read_b + 1u] - beg_b;
    }
    return ok;
}

__global__ void __launch_bounds__(256) k_cigar_plan(CigarArgs p) {
    const AlignArgs &a = p.a;
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c < a.n_chains; c += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_chain rec = a.chains[c];
        uint64_t beg_a, beg_b, rows = 0;
        if (!cigar_record_ok(a, rec, beg_a, beg_b)) {
            a.info[0] = 1u;
        } else {
            const uint32_t m = rec.a_end - rec.a_start, n = rec.b_end - rec.b_start, nd = align_n_diags(m, n, a.band);
            if (nd <= KMU_ALIGN_MAX_DIAGS) {
                rows = align_trace_rows(align_geom(m, n, a.band).steps, align_pairs_per_lane(nd));
                if (rows > p.budget_rows) rows = 0;
            }
        }
        p.rows[c] = (uint32_t) rows; // (budget_rows is below 2^32)
    }
}

__global__ void __launch_bounds__(64) k_cigar_sweep(CigarArgs p) {
    __shared__ uint32_t win_a[ALIGN_WIN_WORDS], win_b[ALIGN_WIN_WORDS];
    const AlignArgs &a = p.a;
    const uint32_t lane = (uint32_t) lane_id();
    uint32_t bad = 0, refused = 0;
    const uint64_t row0 = p.roff[p.b0];
    for (uint64_t c = p.b0 + blockIdx.x; c < p.b1; c += gridDim.x) {
        const kmu_chain rec = a.chains[c];
        kmu_chain_aln o = {0xFFFFFFFFu, 0u, 0u, 0u};
        uint64_t beg_a, beg_b;
        if (!cigar_record_ok(a, rec, beg_a, beg_b)) { // (the plan has seen it: the call is refused)
            refused = 1;
        } else {
            const uint32_t m = rec.a_end - rec.a_start, n = rec.b_end - rec.b_start;
            o.n_diags = align_n_diags(m, n, a.band);
            if (o.n_diags <= KMU_ALIGN_MAX_DIAGS) {
                const AlignGeom g = align_geom(m, n, a.band);
                SeqView va, vb;
                va.base = a.bases_q;
                va.begin = beg_a + rec.a_start;
                va.len = m;
                va.total = a.off_q[a.n_reads_q];
                va.packed = 0;
                vb.base = a.bases_db;
                vb.begin = beg_b + rec.b_start;
                vb.len = n;
                vb.total = a.off_db[a.n_reads_db];
                vb.packed = 0;
                const uint64_t r0 = p.roff[c], rows = p.roff[c + 1] - r0;
                uint32_t *slab = p.trace + (r0 - row0) * 64u;
                uint64_t r;
                if (rows) {
                    if (g.n_diags <= 128u) r = align_chain<1, true>(g, va, vb, rec.strand, win_a, win_b, bad, slab);
                    else if (g.n_diags <= 256u) r = align_chain<2, true>(g, va, vb, rec.strand, win_a, win_b, bad, slab);
                    else if (g.n_diags <= 512u) r = align_chain<4, true>(g, va, vb, rec.strand, win_a, win_b, bad, slab);
                    else r = align_chain<8, true>(g, va, vb, rec.strand, win_a, win_b, bad, slab);
                } else { // above the budget: aligned as kmu_chain_align aligns it
                    if (g.n_diags <= 128u) r = align_chain<1>(g, va, vb, rec.strand, win_a, win_b, bad);
                    else if (g.n_diags <= 256u) r = align_chain<2>(g, va, vb, rec.strand, win_a, win_b, bad);
                    else if (g.n_diags <= 512u) r = align_chain<4>(g, va, vb, rec.strand, win_a, win_b, bad);
                    else r = align_chain<8>(g, va, vb, rec.strand, win_a, win_b, bad);
                }
                o.edit = (uint32_t) (r >> 32);
                o.matches = ~(uint32_t) r;
                o.flags = KMU_ALN_DONE | (o.edit - (m > n ? m - n : n - m) <= 2u * a.band ? KMU_ALN_EXACT : 0u) | (rows ? KMU_ALN_PATH : 0u);
            }
        }
        if (lane == 0) a.out[c] = o;
    }
    if (refused && lane == 0) a.info[0] = 1u;
    if (bad) a.info[1] = 1u;
}

// the runs of one chain, written downwards from the end of its slab; returns their number (uniform)
template <int C>
__device__ __forceinline__ uint32_t cigar_walk_chain(const AlignGeom &g, uint32_t *slab, uint32_t rows, uint32_t *blk) {
    const uint32_t lane = (uint32_t) lane_id();
    uint32_t blk_lo = rows, count = 0; // nothing is staged yet: every row is below blk_lo
    uint32_t *const top = slab + (uint64_t) rows * 64u;
    auto read = [&](const AlignSlot &s) -> uint32_t {
        if (s.row < blk_lo) { // (uniform) rows blk_lo .. blk_lo + ALIGN_WALK_ROWS - 1, the last of them s.row
            blk_lo = align_walk_block(s.row);
            __syncthreads(); // the reads of the block before are done
            for (uint32_t r = 0; r < ALIGN_WALK_ROWS && blk_lo + r <= s.row; r++) blk[r * 64u + lane] = slab[(uint64_t) (blk_lo + r) * 64u + lane];
            __syncthreads();
        }
        const uint32_t w = blk[(s.row - blk_lo) * 64u + s.lane];
        return (uint32_t) __builtin_amdgcn_readfirstlane((int) ((w >> s.shift) & 3u));
    };
    auto emit = [&](uint32_t run) {
        count++;
        if (lane == 0) top[-(int64_t) count] = run;
    };
    align_walk<C>(g, read, emit);
    return count;
}

__global__ void __launch_bounds__(64) k_cigar_walk(CigarArgs p) {
    __shared__ uint32_t blk[ALIGN_WALK_ROWS * 64];
    const AlignArgs &a = p.a;
    const uint64_t row0 = p.roff[p.b0];
    for (uint64_t c = p.b0 + blockIdx.x; c < p.b1; c += gridDim.x) {
        const uint64_t r0 = p.roff[c];
        const uint32_t rows = (uint32_t) (p.roff[c + 1] - r0);
        uint32_t count = 0;
        if (rows) { // the plan took the record and the sweep left its bits
            const kmu_chain rec = a.chains[c];
            const AlignGeom g = align_geom(rec.a_end - rec.a_start, rec.b_end - rec.b_start, a.band);
            uint32_t *slab = p.trace + (r0 - row0) * 64u;
            // (a slab's stores and loads are ordered by the kernel boundary between the sweep and the walk)
            if (g.n_diags <= 128u) count = cigar_walk_chain<1>(g, slab, rows, blk);
            else if (g.n_diags <= 256u) count = cigar_walk_chain<2>(g, slab, rows, blk);
            else if (g.n_diags <= 512u) count = cigar_walk_chain<4>(g, slab, rows, blk);
            else count = cigar_walk_chain<8>(g, slab, rows, blk);
        }
        if (lane_id() == 0) p.cnt[c] = count;
    }
}

struct CigarCopyArgs { // every array begins at the batch's first chain
    const uint32_t *cnt;
    const uint64_t *runoff; // [nb + 1]: the scan of cnt
    const uint64_t *roff;   // [nb + 1]
    const uint32_t *trace;
    uint64_t *base;         // [0]: the runs of the batches before; [1]: with this one
    uint32_t *ops;          // null: count only
    uint64_t cap;
    uint64_t *op_off;       // [nb + 1]
    uint64_t nb;
};

__global__ void __launch_bounds__(256) k_cigar_copy(CigarCopyArgs p) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t before = p.base[0];
    for (uint64_t t = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); t < p.nb; t += (uint64_t) gridDim.x * 4u) {
        const uint32_t n = p.cnt[t];
        const uint64_t off = before + p.runoff[t];
        if (lane == 0) p.op_off[t] = off;
        if (!p.ops || !n) continue;
        const uint32_t *src = p.trace + (p.roff[t + 1] - p.roff[0]) * 64u - n; // the last n words of the slab
        for (uint32_t k = lane; k < n; k += 64)
            if (off + k < p.cap) p.ops[off + k] = src[k];
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) p.base[1] = p.op_off[p.nb] = before + p.runoff[p.nb];
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_chain_cigar(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const uint8_t *bases_q,
                               const uint64_t *offsets_q, uint32_t n_reads_q, const uint8_t *bases_db, const uint64_t *offsets_db,
                               uint32_t n_reads_db, const kmu_cigar_params *p, int mem, kmu_chain_aln *aln_out,
                               uint64_t *op_offsets_out, uint32_t *ops_out, uint64_t cap, uint64_t *n_ops_out) {
    if (!ctx || !chains || !bases_q || !offsets_q || !bases_db || !offsets_db || !p || !aln_out || !op_offsets_out || !n_ops_out)
        return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    if (p->band > (KMU_ALIGN_MAX_DIAGS - 1u) / 2u)
        return fail(ctx, KMU_E_BAD_ARG, "band = %u: 2 band + 1 is above KMU_ALIGN_MAX_DIAGS = %d", p->band, KMU_ALIGN_MAX_DIAGS);
    KMU_TRY(check_mem(ctx, mem));
    *n_ops_out = 0;
    if (n_chains == 0) {
        KMU_HIP(ctx, hipSetDevice(ctx->device));
        KMU_TRY(zero_first_offset(ctx, op_offsets_out, mem));
        if (mem == KMU_MEM_DEVICE) KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return KMU_OK;
    }
    if (n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "chains but no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    CigarArgs c{};
    AlignArgs &a = c.a;
    KMU_TRY(stage_to_device(ctx, "cigar.chains", chains, (size_t) n_chains, mem, &a.chains));
    a.n_chains = n_chains;
    KMU_TRY(stage_to_device(ctx, "cigar.basesq", bases_q, mem == KMU_MEM_HOST ? (size_t) offsets_q[n_reads_q] : 0, mem, &a.bases_q));
    KMU_TRY(stage_to_device(ctx, "cigar.offq", offsets_q, (size_t) n_reads_q + 1, mem, &a.off_q));
    if (bases_db == bases_q && offsets_db == offsets_q && n_reads_db == n_reads_q) { // a self-join is staged once
        a.bases_db = a.bases_q;
        a.off_db = a.off_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "cigar.basesdb", bases_db, mem == KMU_MEM_HOST ? (size_t) offsets_db[n_reads_db] : 0, mem, &a.bases_db));
        KMU_TRY(stage_to_device(ctx, "cigar.offdb", offsets_db, (size_t) n_reads_db + 1, mem, &a.off_db));
    }
    a.n_reads_q = n_reads_q;
    a.n_reads_db = n_reads_db;
    a.band = p->band;
    KMU_TRY(dev_array(ctx, "cigar.info", 2, &a.info));
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, 8, ctx->stream));
    uint64_t *d_opoff;
    uint32_t *d_ops;
    KMU_TRY(place_output(ctx, "cigar.aln", aln_out, n_chains, mem, &a.out));
    KMU_TRY(place_output(ctx, "cigar.opoff", op_offsets_out, n_chains + 1, mem, &d_opoff));
    KMU_TRY(place_output(ctx, "cigar.ops", ops_out, cap ? cap : 1, mem, &d_ops));

    // the plan: rows per chain, their offsets, and the batches
    const uint64_t budget = p->max_trace_bytes ? p->max_trace_bytes : KMU_CIGAR_TRACE_DEFAULT;
    c.budget_rows = budget / 256u < 0xFFFFFFFFull ? budget / 256u : 0xFFFFFFFFull;
    uint64_t *d_roff;
    KMU_TRY(dev_array(ctx, "cigar.rows", n_chains, &c.rows));
    KMU_TRY(dev_array(ctx, "cigar.roff", n_chains + 1, &d_roff));
    KMU_TRY(dev_array(ctx, "cigar.cnt", n_chains, &c.cnt));
    c.roff = d_roff;
    KMU_TRY(launch(ctx, "k_cigar_plan", k_cigar_plan, dim3(grid_for(ctx, n_chains, 256)), dim3(256), 0, c));
    KMU_TRY(device_scan_u32(ctx, c.rows, n_chains, d_roff));
    std::vector<uint64_t> roff(n_chains + 1);
    uint32_t h_info[2] = {0, 0};
    KMU_TRY(read_back(ctx, {{roff.data(), d_roff, (n_chains + 1) * 8}, {h_info, a.info, sizeof h_info}})); // (the plan comes with the words)
    const char *refused = "a chain names a read that does not exist, a strand above 1, a start behind its end or an end behind the end of "
                          "its read";
    if (h_info[0]) return refuse(ctx, KMU_E_UNSUPPORTED, "%s", refused);
    std::vector<uint64_t> cuts{0}; // batch k: the chains cuts[k] .. cuts[k + 1] - 1; a chain's own rows are within the budget
    uint64_t max_rows = 1, max_nb = 0;
    for (uint64_t b0 = 0; b0 < n_chains;) {
        uint64_t b1 = b0 + 1;
        while (b1 < n_chains && roff[b1 + 1] - roff[b0] <= c.budget_rows) b1++;
        if (roff[b1] - roff[b0] > max_rows) max_rows = roff[b1] - roff[b0];
        if (b1 - b0 > max_nb) max_nb = b1 - b0;
        cuts.push_back(b1);
        b0 = b1;
    }
    const size_t n_batches = cuts.size() - 1;
    uint64_t *d_base, *d_runoff;
    KMU_TRY(dev_buf(ctx, "cigar.trace", (size_t) max_rows * 256u, (void **) &c.trace));
    KMU_TRY(dev_array(ctx, "cigar.base", n_batches + 1, &d_base));
    KMU_TRY(dev_array(ctx, "cigar.runoff", max_nb + 1, &d_runoff));
    KMU_HIP(ctx, hipMemsetAsync(d_base, 0, 8, ctx->stream));

    for (size_t k = 0; k < n_batches; k++) {
        c.b0 = cuts[k];
        c.b1 = cuts[k + 1];
        const uint64_t nb = c.b1 - c.b0;
        KMU_TRY(launch(ctx, "k_cigar_sweep", k_cigar_sweep, dim3(grid_for(ctx, nb, 1, 16)), dim3(64), 0, c)); // (one-wave workgroups)
        KMU_TRY(launch(ctx, "k_cigar_walk", k_cigar_walk, dim3(grid_for(ctx, nb, 1, 16)), dim3(64), 0, c));
        KMU_TRY(device_scan_u32(ctx, c.cnt + c.b0, nb, d_runoff));
        CigarCopyArgs cp{c.cnt + c.b0, d_runoff, d_roff + c.b0, c.trace, d_base + k, d_ops, cap, d_opoff + c.b0, nb};
        KMU_TRY(launch(ctx, "k_cigar_copy", k_cigar_copy, dim3(grid_for(ctx, nb, 4)), dim3(256), 0, cp));
    }

    uint64_t total = 0;
    KMU_TRY(bring_output(ctx, aln_out, a.out, n_chains, mem));
    KMU_TRY(bring_output(ctx, op_offsets_out, d_opoff, n_chains + 1, mem));
    KMU_TRY(read_back(ctx, {{&total, d_base + n_batches}, {h_info, a.info, sizeof h_info}}));
    KMU_TRY(finish_synced(ctx));
    if (h_info[0]) return fail(ctx, KMU_E_UNSUPPORTED, "%s", refused);
    if (h_info[1]) return fail(ctx, KMU_E_NON_ACGT, "pattern not a code in alphabet_2b (non-ACGT byte in an aligned segment)");
    *n_ops_out = total;
    if (ops_out && cap < total)
        return fail(ctx, KMU_E_BAD_ARG, "cap = %llu is below the %llu runs", (unsigned long long) cap, (unsigned long long) total);
    if (ops_out && mem == KMU_MEM_HOST && total) {
        KMU_TRY(bring_output(ctx, ops_out, d_ops, total, mem));
        KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    }
    return KMU_OK;
}

// kmu_chain_align.hip -- for every chain record the banded global alignment of the two segments it names, on the device
// (kmu_chain_align; the contract is in include/kmu.h, the recurrence as one lane sees it in kmu_align_core.h, the sweep of one
// chain by one wave -- align_chain, which k_cigar_sweep of kmu_chain_cigar.hip runs too -- in kmu_align_sweep.h).
//
//  k_chain_align  one wave per chain, chains dealt grid-stride in one-wave workgroups.  The wave reads the record (uniform), checks
//                 it -- a record that fails is never used as an index; it raises info[0] and the call is refused at its one
//                 synchronisation -- and, where n_diags fits, sweeps the anti-diagonals two at a time (a PAIR-STEP) with the band in
//                 the lanes: lane l owns the C pairs of adjacent diagonals from pair C l on, C = 1, 2, 4 or 8 by the chain's n_diags
//                 (template instances: the values are register arrays with constant indices, no scratch).  One 64-bit key per
//                 diagonal is the whole state.  Per pair-step a lane takes the last odd diagonal of the lane below and, between
//                 the two phases, the first even diagonal of the lane above: DPP wave shifts, no LDS in the recurrence.
//                 Bases: every ALIGN_CHUNK pair-steps the wave stages the code words both segments can be asked for until the next
//                 staging (80 words of 16 bases each, A forward, B forward or reverse-complemented, non-ACGT bytes inside the
//                 segments raise info[1]) in LDS; a lane keeps 32 codes of each segment in a 64-bit register that shifts by one
//                 code per pair-step and is replaced every ALIGN_REFILL pair-steps by words it asked LDS for one refill earlier.
//                 No address depends on a DP value.
//                 m + n + 1 anti-diagonals are one wave's sequential work: a 50 kb overlap is 50 k pair-steps of one wave.
#include "kmu_align_sweep.h" // align_chain: the sweep itself, shared with k_cigar_sweep

namespace kmu {

static_assert(ALIGN_CHUNK == KMU_ALIGN_CHUNK, "the header names the chunk of kmu_align_core.h");
static_assert(KMU_ALIGN_MAX_DIAGS == 1024, "64 lanes x 8 pairs of diagonals");

__global__ void __launch_bounds__(64) k_chain_align(AlignArgs a) {
    __shared__ uint32_t win_a[ALIGN_WIN_WORDS], win_b[ALIGN_WIN_WORDS];
    const uint32_t lane = (uint32_t) lane_id();
    uint32_t bad = 0, refused = 0;
    for (uint64_t c = blockIdx.x; c < a.n_chains; c += gridDim.x) {
        const kmu_chain rec = a.chains[c];
        kmu_chain_aln o = {0xFFFFFFFFu, 0u, 0u, 0u};
        bool ok = rec.read_a < a.n_reads_q && rec.read_b < a.n_reads_db && rec.strand <= 1u && rec.a_start <= rec.a_end &&
                  rec.b_start <= rec.b_end;
        uint64_t beg_a = 0, beg_b = 0;
        if (ok) {
            beg_a = a.off_q[rec.read_a];
            beg_b = a.off_db[rec.read_b];
            ok = rec.a_end <= a.off_q[rec.read_a + 1u] - beg_a && rec.b_end <= a.off_db[rec.read_b + 1u] - beg_b;
        }
        if (!ok) { // the call is refused at its synchronisation
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
                uint64_t r;
                if (g.n_diags <= 128u) r = align_chain<1>(g, va, vb, rec.strand, win_a, win_b, bad);
                else if (g.n_diags <= 256u) r = align_chain<2>(g, va, vb, rec.strand, win_a, win_b, bad);
                else if (g.n_diags <= 512u) r = align_chain<4>(g, va, vb, rec.strand, win_a, win_b, bad);
                else r = align_chain<8>(g, va, vb, rec.strand, win_a, win_b, bad);
                o.edit = (uint32_t) (r >> 32);
                o.matches = ~(uint32_t) r;
                o.flags = KMU_ALN_DONE | (o.edit - (m > n ? m - n : n - m) <= 2u * a.band ? KMU_ALN_EXACT : 0u);
            }
        }
        if (lane == 0) a.out[c] = o;
    }
    if (refused && lane == 0) a.info[0] = 1u;
    if (bad) a.info[1] = 1u;
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_chain_align(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const uint8_t *bases_q,
                               const uint64_t *offsets_q, uint32_t n_reads_q, const uint8_t *bases_db, const uint64_t *offsets_db,
                               uint32_t n_reads_db, const kmu_align_params *p, int mem, kmu_chain_aln *out) {
    if (!ctx || !chains || !bases_q || !offsets_q || !bases_db || !offsets_db || !p || !out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    if (p->band > (KMU_ALIGN_MAX_DIAGS - 1u) / 2u)
        return fail(ctx, KMU_E_BAD_ARG, "band = %u: 2 band + 1 is above KMU_ALIGN_MAX_DIAGS = %d", p->band, KMU_ALIGN_MAX_DIAGS);
    KMU_TRY(check_mem(ctx, mem));
    if (n_chains == 0) return KMU_OK;
    if (n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "chains but no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    AlignArgs a{};
    KMU_TRY(stage_to_device(ctx, "align.chains", chains, (size_t) n_chains, mem, &a.chains));
    a.n_chains = n_chains;
    KMU_TRY(stage_to_device(ctx, "align.basesq", bases_q, mem == KMU_MEM_HOST ? (size_t) offsets_q[n_reads_q] : 0, mem, &a.bases_q));
    KMU_TRY(stage_to_device(ctx, "align.offq", offsets_q, (size_t) n_reads_q + 1, mem, &a.off_q));
    if (bases_db == bases_q && offsets_db == offsets_q && n_reads_db == n_reads_q) { // a self-join is staged once
        a.bases_db = a.bases_q;
        a.off_db = a.off_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "align.basesdb", bases_db, mem == KMU_MEM_HOST ? (size_t) offsets_db[n_reads_db] : 0, mem, &a.bases_db));
        KMU_TRY(stage_to_device(ctx, "align.offdb", offsets_db, (size_t) n_reads_db + 1, mem, &a.off_db));
    }
    a.n_reads_q = n_reads_q;
    a.n_reads_db = n_reads_db;
    a.band = p->band;
    KMU_TRY(dev_array(ctx, "align.info", 2, &a.info));
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, 8, ctx->stream));
    KMU_TRY(place_output(ctx, "align.out", out, n_chains, mem, &a.out));

    KMU_TRY(launch(ctx, "k_chain_align", k_chain_align, dim3(grid_for(ctx, n_chains, 1, 16)), dim3(64), 0, a)); // (one-wave workgroups)
    uint32_t h_info[2] = {0, 0};
    KMU_TRY(bring_output(ctx, out, a.out, n_chains, mem));
    KMU_TRY(read_back(ctx, {{h_info, a.info, sizeof h_info}}));
    KMU_TRY(finish_synced(ctx));
    if (h_info[0])
        return fail(ctx, KMU_E_UNSUPPORTED, "a chain names a read that does not exist, a strand above 1, a start behind its end or an end "
                                            "behind the end of its read");
    if (h_info[1]) return fail(ctx, KMU_E_NON_ACGT, "pattern not a code in alphabet_2b (non-ACGT byte in an aligned segment)");
    return KMU_OK;
}

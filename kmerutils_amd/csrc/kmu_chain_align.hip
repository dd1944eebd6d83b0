// kmu_chain_align.hip -- for every chain record the banded global alignment of the two segments it names, on the device
// (kmu_chain_align; the contract is in include/kmu.h, the recurrence as one lane sees it in kmu_align_core.h).
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
#include "kmu_align_core.h"
#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

static_assert(ALIGN_CHUNK == KMU_ALIGN_CHUNK, "the header names the chunk of kmu_align_core.h");
static_assert(KMU_ALIGN_MAX_DIAGS == 1024, "64 lanes x 8 pairs of diagonals");

struct AlignArgs {
    const kmu_chain *chains;
    uint64_t n_chains;
    const uint8_t *bases_q, *bases_db;
    const uint64_t *off_q, *off_db;
    uint32_t n_reads_q, n_reads_db, band;
    uint32_t *info; // [0]: a record was refused; [1]: a non-ACGT byte inside a segment
    kmu_chain_aln *out;
};

// lane l takes the value of lane l - 1 (wave_shr:1) or l + 1 (wave_shl:1); the lane without a neighbour takes `fill`
__device__ __forceinline__ uint64_t wave_from_below_u64(uint64_t v, uint64_t fill, uint32_t lane) {
    const uint32_t hi = (uint32_t) __builtin_amdgcn_update_dpp((int) (fill >> 32), (int) (v >> 32), 0x138, 0xf, 0xf, false);
    const uint32_t lo = (uint32_t) __builtin_amdgcn_update_dpp((int) (uint32_t) fill, (int) (uint32_t) v, 0x138, 0xf, 0xf, false);
    return lane == 0 ? fill : ((uint64_t) hi << 32) | lo;
}
__device__ __forceinline__ uint64_t wave_from_above_u64(uint64_t v, uint64_t fill, uint32_t lane) {
    const uint32_t hi = (uint32_t) __builtin_amdgcn_update_dpp((int) (fill >> 32), (int) (v >> 32), 0x130, 0xf, 0xf, false);
    const uint32_t lo = (uint32_t) __builtin_amdgcn_update_dpp((int) (uint32_t) fill, (int) (uint32_t) v, 0x130, 0xf, 0xf, false);
    return lane == 63 ? fill : ((uint64_t) hi << 32) | lo;
}

// word k (may lie outside the stream: 0) of a segment's stream; bad: its non-ACGT bytes inside the segment
__device__ __forceinline__ uint32_t align_stream_word(const SeqView &v, const AlignStream &s, uint32_t strand, int32_t k, uint32_t &bad) {
    bad = 0;
    if (k < 0 || (uint32_t) k >= s.n_words) return 0;
    const uint32_t w = load_code_word(v, strand ? s.n_words - 1u - (uint32_t) k : (uint32_t) k, bad);
    return strand ? ~w : align_rev16(w);
}

// the key of cell (m, n), in every lane
template <int C>
__device__ __forceinline__ uint64_t align_chain(const AlignGeom &g, const SeqView &va, const SeqView &vb, uint32_t strand,
                                                uint32_t *win_a, uint32_t *win_b, uint32_t &bad) {
    const uint32_t lane = (uint32_t) lane_id();
    const AlignStream sa = align_stream(seq_lead(va), g.m, 0), sb = align_stream(seq_lead(vb), g.n, strand);
    uint64_t ve[C], vo[C];
#pragma unroll
    for (int c = 0; c < C; c++) ve[c] = vo[c] = ALN_INF;
    const uint32_t e0 = 2u * C * lane;
    uint32_t i0 = (uint32_t) g.I0 - C * lane, j0 = (uint32_t) g.J0 + C * lane; // the even cell of pair 0 at pair-step 0
    for (uint32_t u0 = 0, chunk = 0; u0 < g.steps; u0 += ALIGN_CHUNK, chunk++) { // (uniform)
        const int32_t fa = align_first_a<C>(sa, g, chunk), fb = align_first_b(sb, g, chunk);
        __syncthreads(); // the reads of the chunk before are done
        for (uint32_t k = lane; k < ALIGN_WIN_WORDS; k += 64) {
            uint32_t b0, b1;
            win_a[k] = align_stream_word(va, sa, 0, fa + (int32_t) k, b0);
            win_b[k] = align_stream_word(vb, sb, strand, fb + (int32_t) k, b1);
            bad |= b0 | b1;
        }
        __syncthreads();
        const uint32_t uend = g.steps - u0 < ALIGN_CHUNK ? g.steps : u0 + ALIGN_CHUNK;
        uint32_t pa = align_pos_a<C>(sa, g, fa, u0, lane), pb = align_pos_b<C>(sb, g, fb, u0, lane);
        AlignWords na = align_read(win_a, pa), nb = align_read(win_b, pb);
        for (uint32_t ub = u0; ub < uend; ub += ALIGN_REFILL) {
            uint64_t wa = align_window(na, pa), wb = align_window(nb, pb);
            pa += ALIGN_REFILL;
            pb += ALIGN_REFILL;
            na = align_read(win_a, pa); // for the next refill: in flight while this one is used up
            nb = align_read(win_b, pb);
            const uint32_t cnt = uend - ub < ALIGN_REFILL ? uend - ub : ALIGN_REFILL;
            for (uint32_t s = 0; s < cnt; s++) {
                const uint64_t from_left = wave_from_below_u64(vo[C - 1], ALN_INF, lane);
                align_even<C>(ve, vo, from_left, wa, wb, i0, j0, e0, g);
                const uint64_t from_right = wave_from_above_u64(ve[0], ALN_INF, lane);
                align_odd<C>(ve, vo, from_right, wa, wb, i0, j0, e0, g);
                wa >>= 2;
                wb >>= 2;
                i0++;
                j0++;
            }
        }
    }
    // diagonal ef of lane ef / 2 C
    const uint32_t kf = g.ef % (2u * C), lf = g.ef / (2u * C);
    uint64_t r = ALN_INF;
#pragma unroll
    for (int c = 0; c < C; c++) {
        if (kf == 2u * (uint32_t) c) r = ve[c];
        if (kf == 2u * (uint32_t) c + 1u) r = vo[c];
    }
    return ((uint64_t) readlane_u32((uint32_t) (r >> 32), lf) << 32) | readlane_u32((uint32_t) r, lf);
}

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
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    if (n_chains == 0) return KMU_OK;
    if (n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "chains but no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    AlignArgs a{};
    const void *d;
    KMU_TRY(stage_to_device(ctx, "align.chains", chains, (size_t) n_chains * sizeof(kmu_chain), mem, &d));
    a.chains = (const kmu_chain *) d;
    a.n_chains = n_chains;
    KMU_TRY(stage_to_device(ctx, "align.basesq", bases_q, mem == KMU_MEM_HOST ? (size_t) offsets_q[n_reads_q] : 0, mem, &d));
    a.bases_q = (const uint8_t *) d;
    KMU_TRY(stage_to_device(ctx, "align.offq", offsets_q, ((size_t) n_reads_q + 1) * 8, mem, &d));
    a.off_q = (const uint64_t *) d;
    if (bases_db == bases_q && offsets_db == offsets_q && n_reads_db == n_reads_q) { // a self-join is staged once
        a.bases_db = a.bases_q;
        a.off_db = a.off_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "align.basesdb", bases_db, mem == KMU_MEM_HOST ? (size_t) offsets_db[n_reads_db] : 0, mem, &d));
        a.bases_db = (const uint8_t *) d;
        KMU_TRY(stage_to_device(ctx, "align.offdb", offsets_db, ((size_t) n_reads_db + 1) * 8, mem, &d));
        a.off_db = (const uint64_t *) d;
    }
    a.n_reads_q = n_reads_q;
    a.n_reads_db = n_reads_db;
    a.band = p->band;
    KMU_TRY(dev_array(ctx, "align.info", 2, &a.info));
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, 8, ctx->stream));
    a.out = out;
    if (mem == KMU_MEM_HOST) KMU_TRY(dev_array(ctx, "align.out", n_chains, &a.out));

    KMU_TRY(launch(ctx, "k_chain_align", k_chain_align, dim3(grid_for(ctx, n_chains, 1, 16)), dim3(64), 0, a)); // (one-wave workgroups)
    uint32_t h_info[2] = {0, 0};
    if (mem == KMU_MEM_HOST) KMU_HIP(ctx, hipMemcpyAsync(out, a.out, (size_t) n_chains * sizeof(kmu_chain_aln), hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(h_info, a.info, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->profiling) profile_collect(ctx);
    if (h_info[0])
        return fail(ctx, KMU_E_UNSUPPORTED, "a chain names a read that does not exist, a strand above 1, a start behind its end or an end "
                                            "behind the end of its read");
    if (h_info[1]) return fail(ctx, KMU_E_NON_ACGT, "pattern not a code in alphabet_2b (non-ACGT byte in an aligned segment)");
    return KMU_OK;
}

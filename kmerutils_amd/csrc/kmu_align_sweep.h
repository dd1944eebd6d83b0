// kmu_align_sweep.h -- the forward sweep of one chain by one wave, for the two kernels that run it: k_chain_align
// (kmu_chain_align.hip) and k_cigar_sweep (kmu_chain_cigar.hip).  The recurrence as one lane sees it is in kmu_align_core.h; here are
// the registers, the neighbour lanes' values and the staged code words.  TRACE is a compile-time switch: without it align_chain is
// the sweep of kmu_chain_align and nothing else; with it every lane also writes the two direction bits of each of its cells to the
// chain's slab (layout: kmu_align_core.h).  The stores are fire-and-forget: their addresses come from the loop counters and the
// lane, and nothing the sweep loads or addresses depends on a DP value or on the trace.
#pragma once

#include "kmu_align_core.h"
#include "kmu_ctx.hpp"
#include "kmu_device.h"

namespace kmu {

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

// the key of cell (m, n), in every lane.  TRACE: slab is the chain's align_trace_rows(g.steps, C) rows of 64 words
template <int C, bool TRACE = false>
__device__ __forceinline__ uint64_t align_chain(const AlignGeom &g, const SeqView &va, const SeqView &vb, uint32_t strand,
                                                uint32_t *win_a, uint32_t *win_b, uint32_t &bad, uint32_t *slab = nullptr) {
    const uint32_t lane = (uint32_t) lane_id();
    const AlignStream sa = align_stream(seq_lead(va), g.m, 0), sb = align_stream(seq_lead(vb), g.n, strand);
    uint64_t ve[C], vo[C];
#pragma unroll
    for (int c = 0; c < C; c++) ve[c] = vo[c] = ALN_INF;
    const uint32_t e0 = 2u * C * lane;
    uint32_t i0 = (uint32_t) g.I0 - C * lane, j0 = (uint32_t) g.J0 + C * lane; // the even cell of pair 0 at pair-step 0
    constexpr uint32_t S = 8 / C; // (TRACE) pair-steps per trace word
    static_assert(ALIGN_REFILL % S == 0, "a trace row never spans two refills");
    [[maybe_unused]] uint32_t acc = 0;
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
                [[maybe_unused]] uint32_t bits = 0;
                if constexpr (TRACE) bits = align_even_dirs<C>(ve, vo, from_left, wa, wb);
                align_even<C>(ve, vo, from_left, wa, wb, i0, j0, e0, g);
                const uint64_t from_right = wave_from_above_u64(ve[0], ALN_INF, lane);
                if constexpr (TRACE) {
                    bits |= align_odd_dirs<C>(ve, vo, from_right, wa, wb);
                    acc |= bits << (4u * C * (s % S));
                    if (s % S == S - 1u) { // the word is full: row (ub + s) / S
                        slab[(uint64_t) ((ub + s) / S) * 64u + lane] = acc;
                        acc = 0;
                    }
                }
                align_odd<C>(ve, vo, from_right, wa, wb, i0, j0, e0, g);
                wa >>= 2;
                wb >>= 2;
                i0++;
                j0++;
            }
            if constexpr (TRACE) {
                if (cnt % S) { // the chain's last row, partly filled
                    slab[(uint64_t) ((ub + cnt - 1u) / S) * 64u + lane] = acc;
                    acc = 0;
                }
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

} // namespace kmu

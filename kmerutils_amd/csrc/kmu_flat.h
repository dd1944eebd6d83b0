// kmu_flat.h -- the reads of a batch as ONE flat stream of bases (device code): which read holds a given base, and the wave step
// that every kernel walking the stream is written on (flat_step_visit_words; flat_wave_steps of kmu_count_plan.hpp counts the steps).
#pragma once

#include "kmu_count_plan.hpp"
#include "kmu_device.h"

namespace kmu {

// largest i with offsets[i] <= g, g wave-uniform; 64-ary search, one coalesced probe per round
__device__ __forceinline__ uint32_t wave_find_read(const uint64_t *offsets, uint32_t n, uint64_t g) {
    uint32_t lo = 0, hi = n; // invariant offsets[lo] <= g < offsets[hi]
    const uint32_t lane = (uint32_t) lane_id();
    while (hi - lo > 1) {
        const uint32_t step = (hi - lo + 63) / 64;
        const uint64_t idx = (uint64_t) lo + (uint64_t) (lane + 1) * step;
        const bool le = idx < hi && offsets[idx] <= g;
        const uint32_t c = (uint32_t) __popcll(__ballot(le));
        const uint64_t nhi = (uint64_t) lo + (uint64_t) (c + 1) * step;
        lo = lo + c * step;
        hi = nhi < hi ? (uint32_t) nhi : hi;
    }
    return lo;
}

// the same with a hint: a wave walks the flat stream forwards, so the read is usually one of the next 64
__device__ __forceinline__ uint32_t wave_find_read_from(const uint64_t *offsets, uint32_t n, uint64_t g, uint32_t hint) {
    if (hint >= n || offsets[hint] > g) return wave_find_read(offsets, n, g);
    const uint64_t idx = (uint64_t) hint + 1 + (uint32_t) lane_id();
    const bool le = idx < n && offsets[idx] <= g;
    const uint32_t c = (uint32_t) __popcll(__ballot(le));
    if (c < 64u) return hint + c;
    return wave_find_read(offsets, n, g);
}

// the code words of wave step `st`: this lane's word and (lanes 0/1) the two words after the wave's last
__device__ __forceinline__ void flat_step_load(const uint8_t *bases, uint64_t total, uint64_t st, bool active, uint32_t &w0,
                                               uint32_t &ex, uint32_t *bad_acc = nullptr) {
    w0 = 0;
    ex = 0;
    if (!active) return; // wave-uniform
    SeqView s;
    s.base = bases; s.begin = 0; s.len = total; s.total = total; s.packed = 0;
    uint32_t bad, bad2;
    w0 = load_code_word(s, st * 64 + (uint64_t) lane_id(), bad);
    ex = load_code_word(s, st * 64 + 64 + (uint64_t) (lane_id() & 1), bad2);
    if (bad_acc) *bad_acc |= bad; // (every word is some step's own word: the halo words need no second look)
}

// One wave step (64 words = 1024 bases) of the flat base stream, from its loaded words (flat_step_load): f(j, canon, r) for
// every k-mer start g = (st * 64 + lane) * 16 + j of this lane with g >= lo whose k-mer lies inside one read, g + k <= the end
// of the read r that holds base g.  canon: kmer.reverse_complement().min(kmer), kmercount.rs:938.  The reads occupy
// [offsets[0], total) of the stream; offsets[0] need not be 0 (a range of a larger read set) and callers pass lo >= offsets[0].
// The whole wave calls it.  FAST: a wave whose lanes all sit well inside a read (long reads: most waves) skips the per-k-mer
// boundary tests; r is the lane's read there too.
template <bool FAST, typename F>
__device__ __forceinline__ void flat_step_visit_words(const uint64_t *offsets, uint32_t n_seq, uint64_t total, uint64_t lo, int k,
                                                      uint64_t st, uint32_t w0, uint32_t ex, uint32_t &r_hint, F &&f) {
    uint32_t w1, w2;
    flat_window(w0, ex, w1, w2);
    // the read of the wave's first base (read 0 where the step begins before offsets[0]).  The search wants a base below `total`:
    // a step that begins at or past the end of the stream (no caller's loop gets there) would look for the last base
    uint32_t r = wave_find_read_from(offsets, n_seq, st * 1024 < total ? st * 1024 : total - 1, r_hint);
    r_hint = r;
    const uint64_t g0 = (st * 64 + (uint64_t) lane_id()) * 16;
    const bool in = g0 < total && g0 + 16 > lo;
    uint64_t rend = in ? offsets[r + 1] : 0;
    // on to the read that holds base g.  The last lane's starts may lie at or past `total`, where no read ends beyond g: the
    // bound r + 1 < n_seq stops at the last read and keeps offsets[r + 1] inside the array.
    auto advance = [&](uint64_t g) {
        while (g >= rend && r + 1 < n_seq) { r++; rend = offsets[r + 1]; }
    };
    const uint64_t hi = ((uint64_t) w0 << 32) | w1;
    const int sh = 64 - 2 * k;
    auto canon = [&](int j) {
        const uint64_t val = ((hi << (2 * j)) | (((uint64_t) w2 << (2 * j)) >> 32)) >> sh, rc = revcomp_val(val, k);
        return rc < val ? rc : val;
    };
    if (FAST) {
        if (in) advance(g0); // the read of this lane's first base
        if (__all(!in || (g0 >= lo && rend - g0 >= (uint64_t) (15 + k)))) {
            if (in) {
#pragma unroll
                for (int j = 0; j < 16; j++) f(j, canon(j), r);
            }
            return;
        }
    }
    if (in) {
#pragma unroll
        for (int j = 0; j < 16; j++) {
            const uint64_t g = g0 + j;
            advance(g);
            if (g >= lo && g + k <= rend) f(j, canon(j), r);
        }
    }
}

// the same from the bases: load + visit.  Returns a non-zero mask if this lane saw a non-ACGT byte.
template <bool FAST, typename F>
__device__ __forceinline__ uint32_t flat_step_visit(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, uint64_t total,
                                                    uint64_t lo, int k, uint64_t st, uint32_t &r_hint, F &&f) {
    uint32_t w0, ex, bad = 0;
    flat_step_load(bases, total, st, true, w0, ex, &bad);
    flat_step_visit_words<FAST>(offsets, n_seq, total, lo, k, st, w0, ex, r_hint, f);
    return bad;
}

// f(canon) for every k-mer of the step
template <typename F>
__device__ __forceinline__ uint32_t flat_step_canon(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                                    uint64_t total, uint64_t start, int k, uint64_t st, uint32_t &r_hint, F &&f) {
    return flat_step_visit<true>(bases, offsets, n_seq, total, start, k, st, r_hint, [&](int, uint64_t canon, uint32_t) { f(canon); });
}

} // namespace kmu

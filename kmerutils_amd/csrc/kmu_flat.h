// kmu_flat.h -- the reads of a batch as ONE flat stream of bases (device code): which read holds a given base, and the wave step
// that every kernel walking the stream is written on (flat_step_visit_words; flat_wave_steps of kmu_count_plan.hpp counts the steps),
// with its prefetching halves (flat_step_fetch / flat_step_words) and the two callbacks that collect a lane's k-mers as tile items.
#pragma once

#include "kmu_count_plan.hpp"
#include "kmu_count_table.h" // CKEY_EMPTY, the "no k-mer" mark of flat_step_items
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

// The non-ACGT bits of the 16-base word at flat position g0 that are the call's, the first read starting at `lo`: the stream of a
// device range `offsets + first` begins up to 1023 bases before its first read (flat_stream_extent), and what lies there belongs to
// reads the call was not given -- staged host input never holds them.  Callers ask only for the steps that begin before `lo`
// (wave-uniform: the first step of a stream, the first two of the super-k-mer walk).  Behind the last read nothing is to be done:
// load_code_word keeps the bits below `total`, and the prefetched form is taken only where every word of the step is whole.
__device__ __forceinline__ uint32_t bad_from(uint32_t bad, uint64_t g0, uint64_t lo) {
    const uint32_t lead = lo > g0 ? (lo - g0 < 16 ? (uint32_t) (lo - g0) : 16u) : 0u;
    return bad & ~((1u << lead) - 1u);
}

// the code words of wave step `st`: this lane's word and (lanes 0/1) the two words after the wave's last; bad_acc collects the
// non-ACGT bytes of the lane's word at or behind flat position `lo`
__device__ __forceinline__ void flat_step_load(const uint8_t *bases, uint64_t total, uint64_t st, bool active, uint32_t &w0,
                                               uint32_t &ex, uint32_t *bad_acc = nullptr, uint64_t lo = 0) {
    w0 = 0;
    ex = 0;
    if (!active) return; // wave-uniform
    SeqView s;
    s.base = bases; s.begin = 0; s.len = total; s.total = total; s.packed = 0;
    uint32_t bad, bad2;
    w0 = load_code_word(s, st * 64 + (uint64_t) lane_id(), bad);
    ex = load_code_word(s, st * 64 + 64 + (uint64_t) (lane_id() & 1), bad2);
    if (!bad_acc) return;
    if (st * 1024 < lo) bad = bad_from(bad, (st * 64 + (uint64_t) lane_id()) * 16, lo);
    *bad_acc |= bad; // (every word is some step's own word: the halo words need no second look)
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

// the same from the bases: load + visit.  Returns a non-zero mask if this lane saw a non-ACGT byte at or behind `lo`.
template <bool FAST, typename F>
__device__ __forceinline__ uint32_t flat_step_visit(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, uint64_t total,
                                                    uint64_t lo, int k, uint64_t st, uint32_t &r_hint, F &&f) {
    uint32_t w0, ex, bad = 0;
    flat_step_load(bases, total, st, true, w0, ex, &bad, lo);
    flat_step_visit_words<FAST>(offsets, n_seq, total, lo, k, st, w0, ex, r_hint, f);
    return bad;
}

// f(canon) for every k-mer of the step
template <typename F>
__device__ __forceinline__ uint32_t flat_step_canon(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                                    uint64_t total, uint64_t start, int k, uint64_t st, uint32_t &r_hint, F &&f) {
    return flat_step_visit<true>(bases, offsets, n_seq, total, start, k, st, r_hint, [&](int, uint64_t canon, uint32_t) { f(canon); });
}

// flat_step_load in two halves, for prefetching: flat_step_fetch requests the two aligned 16-byte chunks (this lane's word, the
// halo word of lane & 1) and the lane's 16 "no k-mer" bits (flat_novalid, kmu_smer.hpp), and nothing looks at them until
// flat_step_words turns them into code words one tile later -- the requests are UNCONDITIONAL loads from clamped addresses
// (needs total >= 16), so that their number in flight is a constant for the compiler's s_waitcnt placement (a load under a
// branch makes it wait for everything at the first use of anything).  All vector-memory waits of the scatter loop that uses them
// (k_part_scatter1) are explicit waits for vmcnt(0): once before the loop, once per tile just before the write-out, when the requests
// of the next tile have had the whole tile sort to arrive and the stores of the last tile are long gone.
struct FlatRaw {
    uint4 c0, cx;
    uint32_t nv;
};
__device__ __forceinline__ void flat_step_fetch(const uint8_t *bases, uint64_t total, uint64_t st, FlatRaw &r, const uint16_t *novalid, uint64_t last_step) {
    r.c0 = make_uint4(0u, 0u, 0u, 0u);
    r.cx = r.c0;
    r.nv = novalid[(st < last_step ? st : last_step) * 64 + (uint64_t) lane_id()];
    if (total < 16) return; // (wave-uniform; flat_step_words then reads the ragged chunk itself)
    const uint64_t lastc = (total - 16) & ~15ull;
    const uint64_t a0 = (st * 64 + (uint64_t) lane_id()) * 16, ax = (st * 64 + 64 + (uint64_t) (lane_id() & 1)) * 16;
    r.c0 = *reinterpret_cast<const uint4 *>(bases + (a0 < lastc ? a0 : lastc));
    r.cx = *reinterpret_cast<const uint4 *>(bases + (ax < lastc ? ax : lastc));
}
__device__ __forceinline__ void flat_step_words(const uint8_t *bases, uint64_t total, uint64_t lo, uint64_t st, bool active, const FlatRaw &r,
                                                uint32_t &w0, uint32_t &ex, uint32_t &bad_acc) {
    w0 = 0;
    ex = 0;
    if (!active) return; // wave-uniform
    const uint64_t i0 = st * 64 + (uint64_t) lane_id(), ix = st * 64 + 64 + (uint64_t) (lane_id() & 1);
    uint32_t bad = 0, bad2 = 0;
    if (__all(ix * 16 + 16 <= total)) { // (every chunk of the step whole: all but the last step of the stream)
        w0 = pack16_ascii(r.c0, bad);
        ex = pack16_ascii(r.cx, bad2);
    } else {
        SeqView s;
        s.base = bases; s.begin = 0; s.len = total; s.total = total; s.packed = 0;
        w0 = load_code_word(s, i0, bad);
        ex = load_code_word(s, ix, bad2);
    }
    if (st * 1024 < lo) bad = bad_from(bad, i0 * 16, lo); // (the stream's first step)
    bad_acc |= bad; // (every word is some step's own word: the halo words need no second look)
}

// up to 16 canonical k-mers of this lane for wave step `st` (CKEY_EMPTY where a k-mer would straddle a read end); the exact levels
__device__ __forceinline__ void flat_step_items(const uint64_t *offsets, uint32_t n_seq, uint64_t total, uint64_t start, int k,
                                                uint64_t st, bool active, uint32_t w0, uint32_t ex, uint32_t &r_hint, uint64_t (&it)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j++) it[j] = CKEY_EMPTY;
    if (!active) return; // wave-uniform
    // (the step keeps the reverse complement per k-mer: the exact levels' kernel has no registers for the window's)
    flat_step_visit_words<true>(offsets, n_seq, total, start, k, st, w0, ex, r_hint, [&](int j, uint64_t canon, uint32_t) { it[j] = canon; });
}

// the same from the lane's "no k-mer" bits: no read offsets, no search, no dependent look-up; a wave whose lanes are all-or-nothing
// (long reads: nearly every wave) skips the per-k-mer tests
__device__ __forceinline__ void flat_step_items_nv(int k, bool active, uint32_t w0, uint32_t ex, uint32_t nv, uint64_t (&it)[16]) {
#pragma unroll
    for (int j = 0; j < 16; j++) it[j] = CKEY_EMPTY;
    if (!active) return; // wave-uniform
    uint32_t w1, w2;
    flat_window(w0, ex, w1, w2);
    const uint32_t V = ~nv & 0xFFFFu;
    const StepWin sw = step_win(w0, w1, w2, k);
    if (__all(V == 0xFFFFu || V == 0u)) {
        if (V) {
#pragma unroll
            for (int j = 0; j < 16; j++) it[j] = step_canonical(sw, j);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 16; j++)
            if ((V >> j) & 1u) it[j] = step_canonical(sw, j);
    }
}

} // namespace kmu

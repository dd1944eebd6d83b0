// kmu_align_core.h -- the banded alignment of kmu_chain_align as one lane sees it: the geometry of a chain, the value of a cell,
// the two phases of a pair-step and the 32-base window a lane reads its bases from.  Plain C++ on plain values: the kernel
// (kmu_align_sweep.h, for kmu_chain_align.hip and kmu_chain_cigar.hip) supplies the registers, the neighbour lanes' values and the
// staged code words; a host program can drive the same functions over 64 simulated lanes.  At the end of the file: the path of
// kmu_chain_cigar -- the direction bits of a cell, where they lie in a chain's trace, and the walk back over them.
//
// Diagonals and pairs.  Diagonal e = (j - i) - lo, 0 <= e < n_diags.  Diagonals 2 p and 2 p + 1 are PAIR p; lane l owns the C
// pairs p = C l .. C l + C - 1 (C = 1, 2, 4, 8: 128, 256, 512, 1024 diagonals in the wave).  A PAIR-STEP u is the two
// anti-diagonals t = t0 + 2 u (the even diagonals are live) and t0 + 2 u + 1 (the odd ones), t0 = 0 or -1 so that t0 + lo is even:
//   even diagonal of pair p: cell (i, j)     i = u + I0 - p, j = u + J0 + p,  I0 = (t0 - lo) / 2, J0 = (t0 + lo) / 2
//   odd diagonal of pair p:  cell (i, j + 1) -- the same row.
// The even cell's left and upper neighbours are the odd diagonals of pairs p - 1 and p as pair-step u - 1 left them, the odd cell's
// are the even diagonals of pairs p and p + 1 of THIS pair-step; the diagonal neighbour is the cell's own diagonal one pair-step
// earlier.  So one value per diagonal is the whole state, and a lane takes one value from its left neighbour before the even phase
// and one from its right neighbour between the phases.
// Value: (edits, -matches) as one 64-bit key, edits << 32 | (2^32 - 1 - matches): the smaller key is the lexicographic minimum.
//   Every in-band cell (i, j) is reached along diagonal 0 and then straight, so its edits are at most max(i, j) < 2^31 and ALN_INF,
//   which is above every value, takes one more edit without wrapping.
// Bases: a lane keeps A[i - 1 - (C - 1) ..] and B'[j - 1 ..] of its pair 0 as 32 two-bit codes each (the lowest index in bits
//   1..0); pair c reads code C - 1 - c of the first and codes c (even cell) and c + 1 (odd cell) of the second; a pair-step shifts
//   both down by one code, and after ALIGN_REFILL pair-steps the windows are read anew -- 16 codes are then still ahead, C + 1 <= 9
//   are needed.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_HD __host__ __device__ __forceinline__
#else
#define KMU_HD inline
#endif

namespace kmu {

constexpr uint32_t ALIGN_CHUNK = 512;    // pair-steps (= bases of either segment) between two stagings; include/kmu.h: KMU_ALIGN_CHUNK
constexpr uint32_t ALIGN_REFILL = 16;    // pair-steps between two reads of a lane's windows
constexpr uint32_t ALIGN_WIN_WORDS = 80; // staged code words (16 bases each) per segment: ALIGN_CHUNK + 64 C + C + 48 bases and slack
constexpr uint64_t ALN_INF = 0xFFFFFFFEFFFFFFFFull;
constexpr uint64_t ALN_EDIT = 1ull << 32;

struct AlignGeom {
    uint32_t m, n, n_diags;
    int32_t lo, I0, J0;
    uint32_t steps; // pair-steps: the last one holds t = m + n
    uint32_t ef;    // the diagonal of cell (m, n)
};

// |n - m| + 2 band + 1; never above 2^31 + KMU_ALIGN_MAX_DIAGS for the bands the call takes
KMU_HD uint32_t align_n_diags(uint32_t m, uint32_t n, uint32_t band) { return (m > n ? m - n : n - m) + 2u * band + 1u; }

// only for n_diags <= KMU_ALIGN_MAX_DIAGS: lo is then above -2^10
KMU_HD AlignGeom align_geom(uint32_t m, uint32_t n, uint32_t band) {
    AlignGeom g;
    g.m = m;
    g.n = n;
    g.n_diags = align_n_diags(m, n, band);
    const int32_t dd = (int32_t) (n - m); // |n - m| < 2^10 here
    g.lo = (dd < 0 ? dd : 0) - (int32_t) band;
    const int32_t t0 = -(g.lo & 1);
    g.I0 = (t0 - g.lo) / 2;
    g.J0 = (t0 + g.lo) / 2; // (even numerators: exact)
    g.steps = (uint32_t) (((uint64_t) m + n + (uint64_t) (-t0)) / 2u + 1u);
    g.ef = (uint32_t) (dd - g.lo);
    return g;
}

// cell (i, j) from its three neighbours; ca, cb: the codes of A[i - 1] and B'[j - 1].  i and j are taken modulo 2^32: a negative
// one is far above m and n.
KMU_HD uint64_t align_cell(uint64_t left, uint64_t up, uint64_t dg, uint32_t ca, uint32_t cb, uint32_t i, uint32_t j, bool inband,
                           const AlignGeom &g) {
    uint64_t s = (left < up ? left : up) + ALN_EDIT;
    const uint64_t d = ca == cb ? dg - 1u : dg + ALN_EDIT;
    uint64_t v = d < s ? d : s;
    if (j == 0) v = ((uint64_t) i << 32) | 0xFFFFFFFFu;
    if (i == 0) v = ((uint64_t) j << 32) | 0xFFFFFFFFu;
    if (!(inband && i <= g.m && j <= g.n)) v = ALN_INF;
    return v;
}

// the even diagonals of a lane's pairs at one pair-step.  from_left: the last odd diagonal of the lane below (ALN_INF for lane 0);
// i0, j0: the even cell of the lane's pair 0; e0 = 2 C lane
template <int C>
KMU_HD void align_even(uint64_t (&ve)[C], const uint64_t (&vo)[C], uint64_t from_left, uint64_t wa, uint64_t wb, uint32_t i0,
                       uint32_t j0, uint32_t e0, const AlignGeom &g) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t ca = (uint32_t) (wa >> (2 * (C - 1 - c))) & 3u, cb = (uint32_t) (wb >> (2 * c)) & 3u;
        ve[c] = align_cell(c ? vo[c ? c - 1 : 0] : from_left, vo[c], ve[c], ca, cb, i0 - (uint32_t) c, j0 + (uint32_t) c,
                           e0 + 2u * (uint32_t) c < g.n_diags, g);
    }
}
// the odd diagonals.  ve: as align_even just left it; from_right: ve[0] of the lane above (ALN_INF for lane 63)
template <int C>
KMU_HD void align_odd(const uint64_t (&ve)[C], uint64_t (&vo)[C], uint64_t from_right, uint64_t wa, uint64_t wb, uint32_t i0,
                      uint32_t j0, uint32_t e0, const AlignGeom &g) {
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t ca = (uint32_t) (wa >> (2 * (C - 1 - c))) & 3u, cb = (uint32_t) (wb >> (2 * (c + 1))) & 3u;
        vo[c] = align_cell(ve[c], c + 1 < C ? ve[c + 1 < C ? c + 1 : 0] : from_right, vo[c], ca, cb, i0 - (uint32_t) c,
                           j0 + (uint32_t) c + 1u, e0 + 2u * (uint32_t) c + 1u < g.n_diags, g);
    }
}

// ---- bases ------------------------------------------------------------------------------------------------------------------
// A segment is a STREAM of code words of 16 bases, the first base of a word in its bits 1..0: base x of the segment is code
// lead + x of the stream, and the stream has n_words words.  A staged window holds the words first .. first + ALIGN_WIN_WORDS - 1
// (first may be negative; a word outside the stream is 0).
struct AlignStream {
    uint32_t lead, n_words;
};
KMU_HD int32_t floor16(int64_t v) { return (int32_t) (v >= 0 ? v / 16 : -((15 - v) / 16)); }
// the first staged word of chunk g (pair-steps g ALIGN_CHUNK ...) for the two segments
template <int C> KMU_HD int32_t align_first_a(const AlignStream &s, const AlignGeom &g, uint32_t chunk) {
    return floor16((int64_t) s.lead + (int64_t) chunk * ALIGN_CHUNK + g.I0 - 65 * C);
}
KMU_HD int32_t align_first_b(const AlignStream &s, const AlignGeom &g, uint32_t chunk) {
    return floor16((int64_t) s.lead + (int64_t) chunk * ALIGN_CHUNK + g.J0 - 1);
}
// the code positions, inside the staged window, of a lane's two windows at pair-step u
template <int C> KMU_HD uint32_t align_pos_a(const AlignStream &s, const AlignGeom &g, int32_t first, uint32_t u, uint32_t lane) {
    return (uint32_t) ((int64_t) s.lead + (int64_t) u + g.I0 - (int64_t) C * lane - C - 16 * (int64_t) first);
}
template <int C> KMU_HD uint32_t align_pos_b(const AlignStream &s, const AlignGeom &g, int32_t first, uint32_t u, uint32_t lane) {
    return (uint32_t) ((int64_t) s.lead + (int64_t) u + g.J0 + (int64_t) C * lane - 1 - 16 * (int64_t) first);
}
// 32 codes from code position pos of a window: three words now, put together when they are needed
struct AlignWords {
    uint32_t w0, w1, w2;
};
KMU_HD AlignWords align_read(const uint32_t *win, uint32_t pos) {
    const uint32_t k = pos >> 4;
    return AlignWords{win[k], win[k + 1], win[k + 2]};
}
KMU_HD uint64_t align_window(const AlignWords &w, uint32_t pos) {
    const uint32_t r = 2u * (pos & 15u);
    const uint64_t lo = ((uint64_t) w.w1 << 32) | w.w0;
    return r ? (lo >> r) | ((uint64_t) w.w2 << (64u - r)) : lo;
}
// a stream word from the 16-base code word of kmu_device.h (first base in bits 31..30).  Forward: word k of the stream is code word
// k with its codes in reverse order.  Reverse complement: the stream runs over the code words backwards, and reversing a word's
// codes twice leaves only the complement.
KMU_HD uint32_t align_rev16(uint32_t w) {
    uint32_t r = w;
    r = ((r & 0x33333333u) << 2) | ((r >> 2) & 0x33333333u);
    r = ((r & 0x0F0F0F0Fu) << 4) | ((r >> 4) & 0x0F0F0F0Fu);
    r = ((r & 0x00FF00FFu) << 8) | ((r >> 8) & 0x00FF00FFu);
    return (r << 16) | (r >> 16);
}
// seg_lead: the code slots in front of the segment's first base in its first code word; len: its bases
KMU_HD AlignStream align_stream(uint32_t seg_lead, uint32_t len, uint32_t strand) {
    AlignStream s;
    s.n_words = (uint32_t) (((uint64_t) seg_lead + len + 15u) / 16u);
    s.lead = strand ? (uint32_t) (16ull * s.n_words - seg_lead - len) : seg_lead;
    return s;
}

// ---- the path (kmu_chain_cigar) ---------------------------------------------------------------------------------------------
// Two bits per cell, from the three neighbour values align_cell takes: the step by which the path that is defined backwards from
// (m, n) leaves the cell -- the first that applies of diagonal (d <= s), up (up <= left), left -- and, for a diagonal, whether the
// two bases are equal.  The bits of a cell in row 0 or column 0 or outside the band are never read: the walk knows its way there.
// Trace: a lane's 4 C bits of a pair-step (pair c: the even cell in bits 4 c + 1 .. 4 c, the odd cell in bits 4 c + 3 .. 4 c + 2)
// fill one 32-bit word over S = 8 / C pair-steps, the earliest in the lowest bits; ROW r of a chain is that word of pair-steps
// r S .. r S + S - 1 for all 64 lanes, 256 bytes at word 64 r + lane of the chain's slab.  S divides ALIGN_REFILL, so a row never
// spans two refills.  A chain's slab is ceil(steps / S) rows.
constexpr uint32_t ALIGN_DIR_EQ = 0, ALIGN_DIR_X = 1, ALIGN_DIR_UP = 2, ALIGN_DIR_LEFT = 3;
constexpr uint32_t ALIGN_WALK_ROWS = 32;             // rows the walk has staged at a time: 256 / C pair-steps
constexpr uint32_t ALIGN_MAX_RUN = (1u << 28) - 1u;  // the longest run one uint32 holds
constexpr uint32_t ALIGN_DIR_OPS = 0x2187u;          // BAM's code of direction d in bits 4 d + 3 .. 4 d: = 7, X 8, I 1 (up), D 2 (left)

KMU_HD uint32_t align_dir(uint64_t left, uint64_t up, uint64_t dg, uint32_t ca, uint32_t cb) {
    const uint64_t s = (left < up ? left : up) + ALN_EDIT;
    const uint64_t d = ca == cb ? dg - 1u : dg + ALN_EDIT;
    return d <= s ? (ca == cb ? ALIGN_DIR_EQ : ALIGN_DIR_X) : (up <= left ? ALIGN_DIR_UP : ALIGN_DIR_LEFT);
}
// the bits of a lane's even cells, from the values align_even is about to replace, and of its odd cells, from those align_even
// left and align_odd is about to replace: the arguments are the ones of the call that follows
template <int C>
KMU_HD uint32_t align_even_dirs(const uint64_t (&ve)[C], const uint64_t (&vo)[C], uint64_t from_left, uint64_t wa, uint64_t wb) {
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t ca = (uint32_t) (wa >> (2 * (C - 1 - c))) & 3u, cb = (uint32_t) (wb >> (2 * c)) & 3u;
        bits |= align_dir(c ? vo[c ? c - 1 : 0] : from_left, vo[c], ve[c], ca, cb) << (4 * c);
    }
    return bits;
}
template <int C>
KMU_HD uint32_t align_odd_dirs(const uint64_t (&ve)[C], const uint64_t (&vo)[C], uint64_t from_right, uint64_t wa, uint64_t wb) {
    uint32_t bits = 0;
#pragma unroll
    for (int c = 0; c < C; c++) {
        const uint32_t ca = (uint32_t) (wa >> (2 * (C - 1 - c))) & 3u, cb = (uint32_t) (wb >> (2 * (c + 1))) & 3u;
        bits |= align_dir(ve[c], c + 1 < C ? ve[c + 1 < C ? c + 1 : 0] : from_right, vo[c], ca, cb) << (4 * c + 2);
    }
    return bits;
}
// the instance a chain's n_diags takes, and the rows of its slab
KMU_HD uint32_t align_pairs_per_lane(uint32_t n_diags) { return n_diags <= 128u ? 1u : n_diags <= 256u ? 2u : n_diags <= 512u ? 4u : 8u; }
KMU_HD uint64_t align_trace_rows(uint32_t steps, uint32_t C) { return ((uint64_t) steps * C + 7u) / 8u; }

// where the bits of the in-band cell (i, j) are
struct AlignSlot {
    uint32_t row, lane, shift;
};
template <int C> KMU_HD AlignSlot align_slot(const AlignGeom &g, uint32_t i, uint32_t j) {
    constexpr uint32_t S = 8 / C;
    const uint32_t e = (uint32_t) ((int32_t) (j - i) - g.lo), p = e >> 1;
    const uint32_t u = i - (uint32_t) g.I0 + p; // the pair-step of row i on pair p
    return AlignSlot{u / S, p / C, (u % S) * 4u * C + 4u * (p % C) + 2u * (e & 1u)};
}
// the first row of the block of ALIGN_WALK_ROWS rows the walk stages when it needs `row` and does not have it: the block ends
// with that row, because the pair-step never increases along the walk
KMU_HD uint32_t align_walk_block(uint32_t row) { return row + 1u > ALIGN_WALK_ROWS ? row + 1u - ALIGN_WALK_ROWS : 0u; }

// The walk from (m, n) to (0, 0).  read(slot): the two bits at a slot; emit(run): the runs, len << 4 | BAM code, the LAST run
// of the path first.  Adjacent runs differ in their code unless a run reached max_run: it is cut there, so in path order the
// remainder comes first and every later piece is max_run long.  At most two cells of a pair-step are on the path.
template <int C, class Read, class Emit>
KMU_HD void align_walk(const AlignGeom &g, Read &&read, Emit &&emit, uint32_t max_run = ALIGN_MAX_RUN) {
    uint32_t i = g.m, j = g.n, op = 0, len = 0;
    while (i | j) {
        uint32_t d, k = 1;
        if (i == 0) {
            d = ALIGN_DIR_LEFT;
            k = j;
        } else if (j == 0) {
            d = ALIGN_DIR_UP;
            k = i;
        } else {
            d = read(align_slot<C>(g, i, j));
        }
        i -= d == ALIGN_DIR_LEFT ? 0u : k;
        j -= d == ALIGN_DIR_UP ? 0u : k;
        while (k) {
            if (len && (d != op || len == max_run)) {
                emit((len << 4) | ((ALIGN_DIR_OPS >> (4u * op)) & 15u));
                len = 0;
            }
            op = d;
            const uint32_t t = k < max_run - len ? k : max_run - len;
            len += t;
            k -= t;
        }
    }
    if (len) emit((len << 4) | ((ALIGN_DIR_OPS >> (4u * op)) & 15u));
}

} // namespace kmu

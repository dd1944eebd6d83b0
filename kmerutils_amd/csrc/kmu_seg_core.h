// kmu_seg_core.h -- the arithmetic of read trimming: what a table row says about its support, when two consecutive rows are linked,
// where a supported segment starts and ends, the summary of a read from its kept segments, and the check of a range of
// kmu_extract_ranges; for the device and for a host compiler alike (tests/cpp/sim_pile_segments.cpp drives these functions over 64
// simulated lanes; the contracts are in include/kmu.h).  The read that holds a row (gather_upper_index) and the arithmetic
// of kmu_extract_ranges' copy are in kmu_gather_core.h.
//
// The row pass works on POSITIONS g = 0 .. n_rows, one more than there are rows: the lane of position g knows row g and row g - 1 and
// decides both "row g starts a run" and "row g - 1 ends a run" (the run's exclusive end is g).  So a lane never needs the row behind
// its own, a tile needs one extra row (the one before its first), and the last row of the batch is closed by position n_rows, which
// is never good.  Starts and ends are emitted in ascending order, so the k-th start and the k-th end belong to one run.
#pragma once

#include "kmu_cons_core.h"

namespace kmu {

constexpr uint32_t SEG_TRIPS = 16;                 // trips of 64 positions a wave makes over its tile
constexpr uint32_t SEG_TILE = 64u * SEG_TRIPS;     // positions per tile
constexpr uint32_t SEG_FLAG_LONGEST = 1u;          // KMU_SEG_LONGEST
constexpr uint32_t SEG_WHOLE = 0, SEG_ENDS = 1, SEG_SPLIT = 2, SEG_NONE = 3; // KMU_TRIM_*

KMU_PILE_HD uint64_t seg_n_tiles(uint64_t n_rows) { return (n_rows + 1u + SEG_TILE - 1u) / SEG_TILE; } // over n_rows + 1 positions

// what the row pass keeps of a row: is it good, and depth - ends clamped at 0 (the lower bound of the partners that span to a neighbour)
struct SegRow {
    uint32_t good;
    uint64_t span;
};
KMU_PILE_HD SegRow seg_row(const uint32_t *row, uint32_t min_depth) {
    const uint64_t depth = cons_depth(row), ends = row[PILE_ENDS];
    SegRow s;
    s.good = depth >= min_depth ? 1u : 0u;
    s.span = depth > ends ? depth - ends : 0ull;
    return s;
}
KMU_PILE_HD SegRow seg_no_row() {
    SegRow s;
    s.good = 0u;
    s.span = 0ull;
    return s;
}
// link(g): rows g - 1 (prev) and g (cur) of one read are both good and one of the two bounds reaches min_span
KMU_PILE_HD bool seg_link(const SegRow &prev, const SegRow &cur, uint32_t min_span) {
    return prev.good && cur.good && (cur.span > prev.span ? cur.span : prev.span) >= min_span;
}
// row g starts a run: it is good and (the first row of a read, or the row before is not good or not linked to it)
KMU_PILE_HD bool seg_is_start(const SegRow &prev, const SegRow &cur, bool marked, uint32_t min_span) {
    return cur.good && (marked || !seg_link(prev, cur, min_span));
}
// row g - 1 ends a run (whose exclusive end is g): it is good and row g starts a run, is not good or does not exist
KMU_PILE_HD bool seg_is_end(const SegRow &prev, const SegRow &cur, bool cur_starts) { return prev.good && (cur_starts || !cur.good); }

// the bit of position g in the bitmap of read starts
KMU_PILE_HD bool seg_marked(const uint64_t *marks, uint64_t g) { return (marks[g >> 6] >> (g & 63u)) & 1ull; }

// the summary of a read from its kept segments in order; add one segment after the other, then finish
struct SegSummary {
    uint32_t n_segs, kept, best_start, best_end, first_start, last_end, best_rank;
};
KMU_PILE_HD SegSummary seg_summary_begin() {
    SegSummary s;
    s.n_segs = s.kept = s.best_start = s.best_end = s.first_start = s.last_end = s.best_rank = 0u;
    return s;
}
KMU_PILE_HD void seg_summary_add(SegSummary &s, uint32_t start, uint32_t end) {
    if (s.n_segs == 0u) s.first_start = start;
    if (end - start > s.best_end - s.best_start) { // (strictly longer: the leftmost among equals stays)
        s.best_start = start;
        s.best_end = end;
        s.best_rank = s.n_segs;
    }
    s.last_end = end;
    s.kept += end - start;
    s.n_segs++;
}
KMU_PILE_HD uint32_t seg_inner_bad(const SegSummary &s) { return s.n_segs ? (s.last_end - s.first_start) - s.kept : 0u; }
KMU_PILE_HD uint32_t seg_class(const SegSummary &s, uint32_t n_bases) {
    if (s.n_segs == 0u) return SEG_NONE;
    if (s.n_segs > 1u) return SEG_SPLIT;
    return s.kept == n_bases ? SEG_WHOLE : SEG_ENDS;
}

// kmu_extract_ranges: a range is usable iff begin <= end <= n_bases; its length, 0 for a range that is not
KMU_PILE_HD bool ext_range_ok(uint64_t begin, uint64_t end, uint64_t n_bases) { return begin <= end && end <= n_bases; }

} // namespace kmu

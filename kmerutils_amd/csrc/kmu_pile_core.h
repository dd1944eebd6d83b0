// kmu_pile_core.h -- the index arithmetic of kmu_chain_pileup and the per-row rule of kmu_pile_call, for the device and for a host
// compiler alike (tests/cpp/sim_chain_pileup.cpp drives these functions over 64 simulated lanes; the contract is in include/kmu.h).
//
// A chain's runs are cut into TILES of PILE_TILE runs.  A run of length L is L COLUMNS, whatever its op: a column of `=` / `X` is
// the cell pair (i, j), a column of `I` a base of A alone, a column of `D` a base of B' alone.  Inside a tile the columns are numbered
// run by run; pile_find_run turns a column number into (run, offset) over the inclusive scan of the tile's run lengths, and
// pile_column turns that into the segment indices the column votes on.  The votes of a run as a whole (INS, INS_BASES) belong to
// the run's first column's owner: pile_run_row_a / pile_run_row_b say which row they fall on, if any.
#pragma once

#include <stdint.h>

#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define KMU_PILE_HD __host__ __device__ __forceinline__
#else
#define KMU_PILE_HD inline
#endif

namespace kmu {

constexpr uint32_t PILE_TILE = 64;   // runs per tile: one per lane
constexpr uint32_t PILE_COLS = 8;    // uint32 per row of a table (KMU_PILE_*)
constexpr uint32_t PILE_OP_I = 1, PILE_OP_D = 2, PILE_OP_EQ = 7, PILE_OP_X = 8; // KMU_CIGAR_*
constexpr uint32_t PILE_DEL = 4, PILE_INS = 5, PILE_INS_BASES = 6, PILE_ENDS = 7;
constexpr uint32_t PILE_CALL_NONE = 7, PILE_CALL_INS = 8, PILE_CALL_DIFF = 16;
constexpr uint32_t PILE_NO_CODE = 5; // the code of a read base outside ACGTacgt: equal to no call

// the bases of A and of B' a run consumes; false: an op outside {I, D, =, X} or a length of 0
KMU_PILE_HD bool pile_run_adv(uint32_t run, uint32_t &da, uint32_t &db) {
    const uint32_t op = run & 15u, len = run >> 4;
    const bool diag = op == PILE_OP_EQ || op == PILE_OP_X;
    da = diag || op == PILE_OP_I ? len : 0u;
    db = diag || op == PILE_OP_D ? len : 0u;
    return len != 0u && (diag || op == PILE_OP_I || op == PILE_OP_D);
}

// the number of tiles of a chain with n_runs runs
KMU_PILE_HD uint64_t pile_n_tiles(uint64_t n_runs) { return (n_runs + PILE_TILE - 1u) / PILE_TILE; }

// the first run r of the tile with col < incl[r]; incl: the inclusive scan of the run lengths of the tile's n runs, col < incl[n - 1]
KMU_PILE_HD uint32_t pile_find_run(const uint64_t *incl, uint32_t n, uint64_t col) {
    uint32_t lo = 0, hi = n - 1u; // the answer is in [lo, hi]
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (col < incl[mid]) hi = mid;
        else lo = mid + 1u;
    }
    return lo;
}

// one column: which base of A (i) and which base of B' (j) it stands on; NONE where it has none
constexpr uint32_t PILE_NONE = 0xFFFFFFFFu;
struct PileCol {
    uint32_t i, j;
};
// (i0, j0): where the run begins; off: the column inside the run
KMU_PILE_HD PileCol pile_column(uint32_t op, uint32_t i0, uint32_t j0, uint32_t off) {
    PileCol c;
    c.i = op == PILE_OP_D ? PILE_NONE : i0 + off;
    c.j = op == PILE_OP_I ? PILE_NONE : j0 + off;
    return c;
}

// base j of B' as a forward position of read b
KMU_PILE_HD uint32_t pile_b_pos(uint32_t strand, uint32_t b_start, uint32_t b_end, uint32_t j) {
    return strand ? b_end - 1u - j : b_start + j;
}

// the A row (segment index) that takes the INS / INS_BASES votes of a run that begins at (i0, j0): a D run lies between A's bases
// i0 - 1 and i0 and votes on i0 - 1; PILE_NONE: no vote
KMU_PILE_HD uint32_t pile_run_row_a(uint32_t op, uint32_t i0) { return op == PILE_OP_D && i0 > 0u ? i0 - 1u : PILE_NONE; }
// the same on B, as an index of B': an I run votes on the base before the gap in read b's FORWARD direction, which is j0 - 1 on
// strand 0 and j0 on strand 1 (B' runs backwards there); n: the length of the B segment
KMU_PILE_HD uint32_t pile_run_row_b(uint32_t op, uint32_t strand, uint32_t j0, uint32_t n) {
    if (op != PILE_OP_I) return PILE_NONE;
    if (strand) return j0 < n ? j0 : PILE_NONE;
    return j0 > 0u ? j0 - 1u : PILE_NONE;
}

// the 2-bit code of an ASCII letter (A 0, C 1, G 2, T 3, case does not matter); PILE_NO_CODE outside ACGTacgt
KMU_PILE_HD uint32_t pile_code(uint32_t c) {
    const uint32_t u = c & 0xDFu;
    if (u != 'A' && u != 'C' && u != 'G' && u != 'T') return PILE_NO_CODE;
    const uint32_t x = (c >> 1) & 3u;
    return x ^ (x >> 1);
}

// kmu_pile_call on one row: the call byte; depth: A + C + G + T + DEL
KMU_PILE_HD uint32_t pile_call_row(const uint32_t *row, uint32_t own_byte, uint32_t min_depth, uint64_t &depth) {
    depth = 0;
    for (uint32_t k = 0; k <= PILE_DEL; k++) depth += row[k];
    if (depth < min_depth) return PILE_CALL_NONE;
    const uint32_t own = pile_code(own_byte);
    uint32_t best = 0;
    for (uint32_t k = 1; k <= PILE_DEL; k++)
        if (row[k] > row[best]) best = k; // the smallest code among the largest counts
    if (own <= PILE_DEL && row[own] == row[best]) best = own;
    return best | (2ull * row[PILE_INS] > depth ? PILE_CALL_INS : 0u) | (best != own ? PILE_CALL_DIFF : 0u);
}

} // namespace kmu

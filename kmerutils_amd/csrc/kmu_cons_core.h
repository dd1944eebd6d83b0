// kmu_cons_core.h -- the arithmetic of read correction: the insertion slots of kmu_pile_ins_plan, the votes of kmu_chain_pile_ins and
// the row rule of kmu_pile_consensus, for the device and for a host compiler alike (tests/cpp/sim_pile_consensus.cpp drives these
// functions over 64 simulated lanes; the contracts are in include/kmu.h).
//
// A row g with ins_len[g] > 0 owns the SLOTS S(g) .. S(g) + ins_len[g] - 1, S being the exclusive prefix sum of ins_len over the
// batch's rows.  Nobody holds S: the rows are cut into BLOCKS of CONS_BLOCK, block_off is the exclusive scan of the blocks' sums
// (8 bytes per 64 rows), and cons_slot_base adds the at most 63 bytes before g inside its block.  A gap run that begins at (i0, j0)
// votes its first letters into the slots of the row pile_run_row_a / pile_run_row_b name, slot k taking the letter cons_ins_src_*
// names.  The consensus of a row is its called letter (or its own byte, or nothing) and then the emitted prefix of its slots.
#pragma once

#include "kmu_pile_core.h"

namespace kmu {

constexpr uint32_t CONS_BLOCK = 64;    // rows per block of the slot index, and per tile of the consensus: one per lane
constexpr uint32_t CONS_MAX_INS = 255; // the most slots one row can get (ins_len is a byte)
constexpr uint32_t CONS_LETTERS = 4;   // uint32 per slot: A C G T

// A + C + G + T + DEL of a table row
KMU_PILE_HD uint64_t cons_depth(const uint32_t *row) {
    uint64_t depth = 0;
    for (uint32_t k = 0; k <= PILE_DEL; k++) depth += row[k];
    return depth;
}

// the slots of a row: 0 without KMU_CALL_INS, otherwise min(max_ins, floor((2 INS_BASES - 1) / depth)) -- the most inserted positions at
// which more than half of the depth can still have a letter; 0 also where a table that no call was made from has depth or INS_BASES 0
KMU_PILE_HD uint32_t cons_slot_count(const uint32_t *row, uint32_t call, uint32_t max_ins) {
    if (!(call & PILE_CALL_INS)) return 0u;
    const uint64_t depth = cons_depth(row), ins_bases = row[PILE_INS_BASES];
    if (depth == 0 || ins_bases == 0) return 0u;
    const uint64_t k = (2ull * ins_bases - 1ull) / depth;
    return (uint32_t) (k < max_ins ? k : max_ins);
}

KMU_PILE_HD uint64_t cons_n_blocks(uint64_t n_rows) { return (n_rows + CONS_BLOCK - 1u) / CONS_BLOCK; }

// S(g): the first slot of row g
KMU_PILE_HD uint64_t cons_slot_base(const uint64_t *block_off, const uint8_t *ins_len, uint64_t g) {
    uint64_t s = block_off[g / CONS_BLOCK];
    for (uint64_t r = g - g % CONS_BLOCK; r < g; r++) s += ins_len[r];
    return s;
}

// how many letters of a gap run of length len are voted on a row with ins_len slots: the others are dropped
KMU_PILE_HD uint32_t cons_ins_votes(uint32_t len, uint32_t ins_len) { return len < ins_len ? len : ins_len; }
// A side, a D run that begins at (i0, j0): slot k takes the letter of B' at this index
KMU_PILE_HD uint32_t cons_ins_src_a(uint32_t j0, uint32_t k) { return j0 + k; }
// B side, an I run of length len that begins at (i0, j0): slot k, counted in read b's forward direction, takes A's letter at this index
KMU_PILE_HD uint32_t cons_ins_src_b(uint32_t strand, uint32_t i0, uint32_t len, uint32_t k) { return strand ? i0 + len - 1u - k : i0 + k; }
// the code a letter votes for: B's forward letter seen from A, or A's letter seen from read b -- complemented on strand 1 both ways
KMU_PILE_HD uint32_t cons_ins_code(uint32_t byte, uint32_t strand) {
    const uint32_t code = pile_code(byte);
    return code == PILE_NO_CODE ? code : strand ? 3u - code : code;
}

// the slots of a row that are emitted: the longest prefix in which every slot holds the votes of more than half of the depth
KMU_PILE_HD uint32_t cons_emitted(const uint32_t *slots, uint32_t ins_len, uint64_t depth) {
    uint32_t k = 0;
    for (; k < ins_len; k++) {
        uint64_t n = 0;
        for (uint32_t x = 0; x < CONS_LETTERS; x++) n += slots[k * CONS_LETTERS + x];
        if (2ull * n <= depth) break;
    }
    return k;
}
// the letter of a slot: the largest count, the smallest code among equals
KMU_PILE_HD uint8_t cons_slot_letter(const uint32_t *slot) {
    uint32_t best = 0;
    for (uint32_t x = 1; x < CONS_LETTERS; x++)
        if (slot[x] > slot[best]) best = x;
    return (uint8_t) "ACGT"[best];
}

// the bytes the row's own position gives: none for a DEL call, otherwise one
KMU_PILE_HD uint32_t cons_own_len(uint32_t call) { return (call & 7u) == PILE_DEL ? 0u : 1u; }
// ... and that byte: the called letter in upper case; the read's own byte, whatever it is, where there is no call
KMU_PILE_HD uint8_t cons_own_byte(uint32_t call, uint32_t own) { return (call & 7u) < PILE_DEL ? (uint8_t) "ACGT"[call & 7u] : (uint8_t) own; }

// the output of one row.  row and slots are looked at only where ins_len > 0 (row: the 8 counts; slots: the row's own, [ins_len][4]);
// out == nullptr counts only.  Returns the number of bytes.
KMU_PILE_HD uint32_t cons_row(uint32_t call, uint32_t own, uint32_t ins_len, const uint32_t *row, const uint32_t *slots, uint8_t *out) {
    uint32_t n = cons_own_len(call);
    if (out && n) out[0] = cons_own_byte(call, own);
    if (ins_len) {
        const uint32_t e = cons_emitted(slots, ins_len, cons_depth(row));
        if (out)
            for (uint32_t k = 0; k < e; k++) out[n + k] = cons_slot_letter(slots + k * CONS_LETTERS);
        n += e;
    }
    return n;
}

} // namespace kmu

// kmu_pile_plan.h -- the host steps the calls over a chain's runs share: kmu_chain_pileup and kmu_chain_pile_ins take the same
// inputs, refuse the same inputs and cut the runs into the same tiles (pile_check_inputs, pile_plan: kmu_chain_pileup.hip);
// kmu_chain_pile_ins and kmu_pile_consensus find the slots of a row through the same block offsets (ins_block_offsets:
// kmu_pile_ins.hip).
#pragma once

#include "kmu_ctx.hpp"
#include "kmu_pile_core.h"

namespace kmu {

struct PileTileRec { // where a tile begins
    uint64_t chain;
    uint32_t i, j;
};

struct PileArgs {
    const kmu_chain *chains;
    const kmu_chain_aln *aln;
    uint64_t n_chains;
    const uint64_t *op_off; // [n_chains + 1]
    const uint32_t *ops;
    uint64_t n_ops;
    const uint8_t *bases_q, *bases_db;
    const uint64_t *off_q, *off_db;
    uint32_t n_reads_q, n_reads_db;
    uint32_t flags;
    uint32_t *pile_q, *pile_db;
    uint32_t *n_tiles;      // [n_chains]
    const uint64_t *tile_off; // [n_chains + 1]
    PileTileRec *tiles;
    uint64_t tile_cap;
    uint32_t *info;         // [0]: refused; [1]: a voted letter outside ACGTacgt
};

// the inputs of a call, as the caller names them
struct PileInputs {
    const kmu_chain *chains;
    uint64_t n_chains;
    const kmu_chain_aln *aln;
    const uint64_t *op_offsets;
    const uint32_t *ops;
    uint64_t n_ops;
    const uint8_t *bases_q;
    const uint64_t *offsets_q;
    uint32_t n_reads_q;
    const uint8_t *bases_db;
    const uint64_t *offsets_db;
    uint32_t n_reads_db;
    const kmu_pileup_params *p;
    int mem;
    bool self() const { return bases_db == bases_q && offsets_db == offsets_q && n_reads_db == n_reads_q; }
};

// the KMU_E_BAD_ARG refusals of the inputs and of the two tables (one per side; of whatever the call votes into)
int pile_check_inputs(kmu_ctx *ctx, const PileInputs &in, const void *table_q, const void *table_db);
// n_chains > 0: stages the inputs, checks every record and run on the device and leaves the tiles (k_pile_count, scan,
// k_pile_starts); one synchronisation; KMU_E_UNSUPPORTED for what kmu_chain_pileup refuses.  a: everything but the tables.
int pile_plan(kmu_ctx *ctx, const PileInputs &in, PileArgs *a, uint64_t *n_tiles);

// the exclusive scan of the sums of ins_len (device memory, n_rows bytes) over blocks of CONS_BLOCK rows: block_off[cons_n_blocks + 1]
// in workspace `name` (and name + ".sum"), its last entry being the number of slots; nothing is synchronised
int ins_block_offsets(kmu_ctx *ctx, const char *name, const uint8_t *ins_len, uint64_t n_rows, uint64_t **block_off);

} // namespace kmu

// kmu_pile_ins.hip -- the inserted letters of the read pileup: how many insertion slots every base gets (kmu_pile_ins_plan) and the
// votes of every chain's gap runs into them (kmu_chain_pile_ins).  The contracts are in include/kmu.h, the arithmetic in
// kmu_cons_core.h; the checks and the tiles are those of kmu_chain_pileup (kmu_pile_plan.h).
//
//  k_ins_plan     one lane per base: a byte load of the call, and only behind KMU_CALL_INS the 32-byte row; ins_len[g] and, one
//                 64-bit atomic add per wave, the number of slots.
//  k_ins_blocks   one wave per block of 64 rows: the sum of their ins_len.  device_scan_u32 turns the sums into block offsets
//                 (8 bytes per 64 rows); S(g) is the offset of g's block plus the at most 63 bytes before g inside it.
//  k_ins_vote     one wave per tile of 64 runs, one run per lane: the DPP scans of k_pile_vote give where the run begins.  Only a
//                 lane that owns a gap run of a voted side goes on: one byte load of ins_len at the run's row, and only where that
//                 is not 0 the lookup of S(g) and at most ins_len letter loads and atomic adds.  Plain uint32 atomicAdd.
#include "kmu_ctx.hpp"
#include "kmu_device.h"
#include "kmu_cons_core.h"
#include "kmu_pile_plan.h"

namespace kmu {

static_assert(CONS_MAX_INS == KMU_INS_MAX && CONS_LETTERS == KMU_INS_COLS && CONS_BLOCK == PILE_TILE, "the slot constants are the header's");

__global__ void __launch_bounds__(256) k_ins_plan(const uint32_t *pile, const uint8_t *call, uint64_t n_bases, uint32_t max_ins, uint8_t *ins_len,
                                                  unsigned long long *n_slots) {
    uint64_t mine = 0;
    for (uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; g < n_bases; g += (uint64_t) gridDim.x * blockDim.x) {
        const uint32_t c = call[g];
        uint32_t n = 0;
        if (c & PILE_CALL_INS) {
            uint32_t row[PILE_COLS];
            for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = pile[g * PILE_COLS + k];
            n = cons_slot_count(row, c, max_ins);
        }
        ins_len[g] = (uint8_t) n;
        mine += n;
    }
    mine = wave_sum_u64(mine);
    if (lane_id() == 0 && mine) atomicAdd(n_slots, (unsigned long long) mine);
}

__global__ void __launch_bounds__(256) k_ins_blocks(const uint8_t *ins_len, uint64_t n_rows, uint64_t n_blocks, uint32_t *sums) {
    const uint32_t lane = (uint32_t) lane_id();
    for (uint64_t b = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); b < n_blocks; b += (uint64_t) gridDim.x * 4u) {
        const uint64_t g = b * CONS_BLOCK + lane;
        const uint32_t s = wave_sum_u32(g < n_rows ? ins_len[g] : 0u);
        if (lane == 0) sums[b] = s;
    }
}

int ins_block_offsets(kmu_ctx *ctx, const char *name, const uint8_t *ins_len, uint64_t n_rows, uint64_t **block_off) {
    const uint64_t n_blocks = cons_n_blocks(n_rows);
    const std::string sum_name = std::string(name) + ".sum";
    uint32_t *sums;
    KMU_TRY(dev_array(ctx, sum_name.c_str(), n_blocks ? n_blocks : 1, &sums));
    KMU_TRY(dev_array(ctx, name, n_blocks + 1, block_off));
    if (n_blocks == 0) {
        KMU_HIP(ctx, hipMemsetAsync(*block_off, 0, 8, ctx->stream));
        return KMU_OK;
    }
    KMU_TRY(launch(ctx, "k_ins_blocks", k_ins_blocks, dim3(grid_for(ctx, n_blocks, 4)), dim3(256), 0, ins_len, n_rows, n_blocks, sums));
    return device_scan_u32(ctx, sums, n_blocks, *block_off);
}

struct InsArgs {
    PileArgs p;                       // the chains, their runs and tiles; the pile tables are not used
    const uint8_t *len_q, *len_db;    // ins_len of the two batches
    const uint64_t *boff_q, *boff_db; // their block offsets
    uint64_t n_slots_q, n_slots_db;
    uint32_t *ins_q, *ins_db;         // [n_slots][4]
};

__global__ void __launch_bounds__(64) k_ins_vote(InsArgs q, uint64_t n_tiles) {
    const PileArgs &p = q.p;
    const uint32_t lane = (uint32_t) lane_id();
    const bool side_q = (p.flags & KMU_PILE_Q) != 0, side_db = (p.flags & KMU_PILE_DB) != 0;
    uint32_t non_acgt = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const PileTileRec tr = p.tiles[t];
        const kmu_chain rec = p.chains[tr.chain];
        const uint64_t first = p.op_off[tr.chain] + (t - p.tile_off[tr.chain]) * PILE_TILE, hi = p.op_off[tr.chain + 1];
        const uint32_t nr = hi - first < PILE_TILE ? (uint32_t) (hi - first) : PILE_TILE;
        const uint32_t m = rec.a_end - rec.a_start, n = rec.b_end - rec.b_start;
        const uint64_t beg_a = p.off_q[rec.read_a] + rec.a_start, beg_b = p.off_db[rec.read_b]; // rows of A's base 0 and of read b's base 0
        const uint8_t *const let_a = p.bases_q + beg_a, *const let_b = p.bases_db + beg_b;

        uint32_t run = 0, da = 0, db = 0;
        if (lane < nr) {
            run = p.ops[first + lane];
            pile_run_adv(run, da, db);
        }
        const uint32_t op = run & 15u, len = run >> 4;
        const uint32_t ia = wave_incl_scan_u32(da), ib = wave_incl_scan_u32(db); // (the chain's sums are m and n: below 2^32)
        const uint32_t i0 = tr.i + ia - da, j0 = tr.j + ib - db;
        if (lane < nr) { // (pile_plan has checked the sums: a run's letters lie inside the segments; the comparisons with m and n never fail)
            const uint32_t ra = pile_run_row_a(op, i0);
            if (side_q && ra != PILE_NONE && ra < m && (uint64_t) j0 + len <= n) {
                const uint64_t g = beg_a + ra;
                const uint32_t il = q.len_q[g];
                if (il) {
                    const uint64_t s = cons_slot_base(q.boff_q, q.len_q, g);
                    const uint32_t votes = s + il <= q.n_slots_q ? cons_ins_votes(len, il) : 0u; // (the sum of ins_len is n_slots: never 0 here)
                    for (uint32_t k = 0; k < votes; k++) {
                        const uint32_t code = cons_ins_code(let_b[pile_b_pos(rec.strand, rec.b_start, rec.b_end, cons_ins_src_a(j0, k))], rec.strand);
                        if (code == PILE_NO_CODE) non_acgt = 1u;
                        else atomicAdd(q.ins_q + (s + k) * CONS_LETTERS + code, 1u);
                    }
                }
            }
            const uint32_t rb = pile_run_row_b(op, rec.strand, j0, n);
            if (side_db && rb != PILE_NONE && rb < n && (uint64_t) i0 + len <= m) {
                const uint64_t g = beg_b + pile_b_pos(rec.strand, rec.b_start, rec.b_end, rb);
                const uint32_t il = q.len_db[g];
                if (il) {
                    const uint64_t s = cons_slot_base(q.boff_db, q.len_db, g);
                    const uint32_t votes = s + il <= q.n_slots_db ? cons_ins_votes(len, il) : 0u;
                    for (uint32_t k = 0; k < votes; k++) {
                        const uint32_t code = cons_ins_code(let_a[cons_ins_src_b(rec.strand, i0, len, k)], rec.strand);
                        if (code == PILE_NO_CODE) non_acgt = 1u;
                        else atomicAdd(q.ins_db + (s + k) * CONS_LETTERS + code, 1u);
                    }
                }
            }
        }
    }
    if (non_acgt) p.info[1] = 1u;
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_pile_ins_plan(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, uint64_t n_bases, const kmu_ins_plan_params *p, int mem,
                                 uint8_t *ins_len_out, uint64_t *n_slots_out) {
    if (!ctx || !pile || !call || !p || !ins_len_out || !n_slots_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->max_ins == 0 || p->max_ins > KMU_INS_MAX) return fail(ctx, KMU_E_BAD_ARG, "max_ins = %u: 1 .. %u", p->max_ins, KMU_INS_MAX);
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    KMU_TRY(check_mem(ctx, mem));
    *n_slots_out = 0;
    if (n_bases == 0) return KMU_OK;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const uint32_t *d_pile;
    const uint8_t *d_call;
    KMU_TRY(stage_to_device(ctx, "insplan.pile", pile, (size_t) n_bases * PILE_COLS, mem, &d_pile));
    KMU_TRY(stage_to_device(ctx, "insplan.call", call, (size_t) n_bases, mem, &d_call));
    uint8_t *d_len;
    KMU_TRY(place_output(ctx, "insplan.len", ins_len_out, n_bases, mem, &d_len));
    unsigned long long *d_total;
    KMU_TRY(dev_array(ctx, "insplan.total", 1, &d_total));
    KMU_HIP(ctx, hipMemsetAsync(d_total, 0, 8, ctx->stream));
    KMU_TRY(launch(ctx, "k_ins_plan", k_ins_plan, dim3(grid_for(ctx, n_bases, 256)), dim3(256), 0, d_pile, d_call, n_bases, p->max_ins, d_len, d_total));
    unsigned long long total = 0;
    KMU_TRY(bring_output(ctx, ins_len_out, d_len, n_bases, mem));
    KMU_TRY(read_back(ctx, {{&total, d_total}}));
    *n_slots_out = total;
    return finish_synced(ctx);
}

extern "C" int kmu_chain_pile_ins(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln, const uint64_t *op_offsets,
                                  const uint32_t *ops, uint64_t n_ops, const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                                  const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db, const kmu_pileup_params *p, int mem,
                                  const uint8_t *ins_len_q, uint64_t n_slots_q, uint32_t *ins_q, const uint8_t *ins_len_db, uint64_t n_slots_db,
                                  uint32_t *ins_db) {
    const PileInputs in{chains, n_chains, aln, op_offsets, ops, n_ops, bases_q, offsets_q, n_reads_q, bases_db, offsets_db, n_reads_db, p, mem};
    KMU_TRY(pile_check_inputs(ctx, in, ins_q, ins_db));
    const bool side_q = p->flags & KMU_PILE_Q, side_db = p->flags & KMU_PILE_DB;
    if ((side_q && !ins_len_q) || (side_db && !ins_len_db)) return fail(ctx, KMU_E_BAD_ARG, "null ins_len for a side that is asked for");
    const bool shared = side_q && side_db && ins_q == ins_db;
    if (shared && (ins_len_q != ins_len_db || n_slots_q != n_slots_db))
        return fail(ctx, KMU_E_BAD_ARG, "one table for both sides needs one ins_len and one n_slots");
    if (n_chains == 0) return KMU_OK;
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    InsArgs a{};
    uint64_t n_tiles = 0;
    KMU_TRY(pile_plan(ctx, in, &a.p, &n_tiles));

    // the bases of the two batches: the size of ins_len
    uint64_t n_bases[2] = {0, 0};
    if (mem == KMU_MEM_HOST) {
        n_bases[0] = offsets_q[n_reads_q];
        n_bases[1] = offsets_db[n_reads_db];
    } else KMU_TRY(read_back(ctx, {{&n_bases[0], offsets_q + n_reads_q}, {&n_bases[1], offsets_db + n_reads_db}}));
    const uint64_t n_bases_q = n_bases[0], n_bases_db = n_bases[1];

    // the slot index of the voted sides, and the refusal of an ins_len that does not belong to n_slots
    uint64_t *boff;
    const uint64_t *sums[2] = {nullptr, nullptr};
    if (side_q) {
        KMU_TRY(stage_to_device(ctx, "ins.lenq", ins_len_q, (size_t) n_bases_q, mem, &a.len_q));
        KMU_TRY(ins_block_offsets(ctx, "ins.boffq", a.len_q, n_bases_q, &boff));
        a.boff_q = boff;
        sums[0] = boff + cons_n_blocks(n_bases_q);
    }
    if (shared) {
        a.len_db = a.len_q;
        a.boff_db = a.boff_q;
    } else if (side_db) {
        KMU_TRY(stage_to_device(ctx, "ins.lendb", ins_len_db, (size_t) n_bases_db, mem, &a.len_db));
        KMU_TRY(ins_block_offsets(ctx, "ins.boffdb", a.len_db, n_bases_db, &boff));
        a.boff_db = boff;
        sums[1] = boff + cons_n_blocks(n_bases_db);
    }
    uint64_t totals[2] = {n_slots_q, n_slots_db};
    KMU_TRY(read_back(ctx, {{&totals[0], sums[0]}, {&totals[1], sums[1]}}));
    const uint64_t total_q = totals[0], total_db = totals[1];
    if (total_q != n_slots_q || total_db != n_slots_db)
        return refuse(ctx, KMU_E_UNSUPPORTED, "ins_len sums to %llu (q) and %llu (db) slots, not to n_slots", (unsigned long long) total_q,
                      (unsigned long long) total_db);
    a.n_slots_q = n_slots_q;
    a.n_slots_db = n_slots_db;
    a.ins_q = side_q ? ins_q : nullptr;
    a.ins_db = side_db ? ins_db : nullptr;
    const size_t words_q = mem == KMU_MEM_HOST && side_q ? (size_t) n_slots_q * CONS_LETTERS : 0;
    const size_t words_db = mem == KMU_MEM_HOST && side_db && !shared ? (size_t) n_slots_db * CONS_LETTERS : 0;
    if (mem == KMU_MEM_HOST) { // the votes of this call alone, added to the caller's tables at the end
        if (side_q) {
            KMU_TRY(dev_array(ctx, "ins.tableq", words_q ? words_q : 1, &a.ins_q));
            KMU_HIP(ctx, hipMemsetAsync(a.ins_q, 0, words_q * 4, ctx->stream));
        }
        if (shared) a.ins_db = a.ins_q;
        else if (side_db) {
            KMU_TRY(dev_array(ctx, "ins.tabledb", words_db ? words_db : 1, &a.ins_db));
            KMU_HIP(ctx, hipMemsetAsync(a.ins_db, 0, words_db * 4, ctx->stream));
        }
    }
    uint32_t h_info[2] = {0, 0};
    if (n_tiles && (n_slots_q || n_slots_db)) KMU_TRY(launch(ctx, "k_ins_vote", k_ins_vote, dim3(grid_for(ctx, n_tiles, 1, 32)), dim3(64), 0, a, n_tiles));
    KMU_TRY(read_back(ctx, {{h_info, a.p.info, sizeof h_info}}));
    KMU_TRY(finish_synced(ctx));
    std::vector<uint32_t> got;
    auto add_down = [&](uint32_t *mine, const uint32_t *dev, size_t words) -> int { // the caller's table += this call's
        got.resize(words);
        if (words) KMU_HIP(ctx, hipMemcpy(got.data(), dev, words * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < words; k++) mine[k] += got[k];
        return KMU_OK;
    };
    if (mem == KMU_MEM_HOST) {
        if (side_q) KMU_TRY(add_down(ins_q, a.ins_q, words_q));
        if (side_db && !shared) KMU_TRY(add_down(ins_db, a.ins_db, words_db));
    }
    if (h_info[1]) return fail(ctx, KMU_E_NON_ACGT, "an inserted letter outside ACGTacgt");
    return KMU_OK;
}

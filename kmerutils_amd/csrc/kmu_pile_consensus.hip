// kmu_pile_consensus.hip -- the corrected reads: the consensus sequence of every read from its calls and its insertion slots
// (kmu_pile_consensus).  The contract is in include/kmu.h, the row rule in kmu_cons_core.h.
//
// Tiles are 64 consecutive rows of the batch, whatever read they belong to; they are the blocks of the slot index, so the first slot
// of a lane's row is its tile's block offset (ins_block_offsets) plus the wave's exclusive scan of ins_len.
//
//  k_cons_count    one wave per tile, one row per lane: the bytes the row gives -- three byte loads (call, ins_len, and in the write
//                  pass the read's own base); the 32-byte pile row and the slots only where ins_len > 0.  Leaves the tile's sum.
//                  device_scan_u32 turns the sums into tile offsets, the last being the total.
//  k_cons_write    the same walk with the wave's prefix sum of the row lengths: every lane stores its row's bytes.
//  k_cons_offsets  one lane per read (and one for the end): cons_offsets[r] is the offset of the tile that holds offsets[r] plus the
//                  lengths of the at most 63 rows before it in that tile.
//  k_cons_pos      (kmu_pile_consensus_pos) the same step, cons_pos_at, for rows a caller names: one lane per query, after
//                  k_cons_pos_check has refused a row above n_rows.
#include "kmu_ctx.hpp"
#include "kmu_device.h"
#include "kmu_cons_core.h"
#include "kmu_pile_plan.h"

namespace kmu {

struct ConsArgs {
    const uint32_t *pile;
    const uint8_t *call, *ins_len;
    const uint32_t *ins;       // [n_slots][4]
    uint64_t n_slots;
    const uint8_t *bases;
    const uint64_t *off;       // [n_reads + 1]
    uint32_t n_reads;
    uint64_t n_rows, n_tiles;
    const uint64_t *slot_off;  // [n_tiles + 1]: the first slot of every tile
    uint32_t *tile_len;        // [n_tiles]: the bytes of every tile
    const uint64_t *tile_off;  // [n_tiles + 1]
    uint64_t *cons_off;        // [n_reads + 1]
    uint8_t *cons;
};

// the bytes of row g, whose slots begin at `slot`; out == nullptr counts only.  A row whose slots would end above n_slots has none
// (the sum of ins_len is n_slots: never taken).
__device__ __forceinline__ uint32_t cons_row_at(const ConsArgs &p, uint64_t g, uint64_t slot, uint8_t *out) {
    const uint32_t call = p.call[g];
    uint32_t il = p.ins_len[g];
    if (slot + il > p.n_slots) il = 0;
    uint32_t row[PILE_COLS] = {};
    if (il)
        for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = p.pile[g * PILE_COLS + k];
    return cons_row(call, out ? p.bases[g] : 0u, il, row, p.ins + slot * CONS_LETTERS, out);
}

template <bool WRITE> __global__ void __launch_bounds__(256) k_cons_tiles(ConsArgs p) {
    const uint32_t lane = (uint32_t) lane_id();
    for (uint64_t t = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); t < p.n_tiles; t += (uint64_t) gridDim.x * 4u) {
        const uint64_t g = t * CONS_BLOCK + lane;
        const bool live = g < p.n_rows;
        const uint32_t il = live ? p.ins_len[g] : 0u;
        const uint64_t slot = p.slot_off[t] + (wave_incl_scan_u32(il) - il);
        const uint32_t n = live ? cons_row_at(p, g, slot, nullptr) : 0u;
        if (!WRITE) {
            const uint32_t sum = wave_sum_u32(n);
            if (lane == 0) p.tile_len[t] = sum;
        } else {
            const uint64_t at = p.tile_off[t] + (wave_incl_scan_u32(n) - n);
            if (n) cons_row_at(p, g, slot, p.cons + at);
        }
    }
}

// the consensus bytes that the rows before row g0 produce: the offset of the tile that holds g0 plus the lengths of the at most 63 rows
// before it in that tile (g0 <= n_rows; t == n_tiles where g0 == n_rows is a multiple of 64: the totals)
__device__ __forceinline__ uint64_t cons_pos_at(const ConsArgs &p, uint64_t g0) {
    const uint64_t t = g0 / CONS_BLOCK;
    uint64_t at = p.tile_off[t], slot = p.slot_off[t];
    for (uint64_t g = t * CONS_BLOCK; g < g0; g++) {
        at += cons_row_at(p, g, slot, nullptr);
        slot += p.ins_len[g];
    }
    return at;
}

__global__ void __launch_bounds__(256) k_cons_offsets(ConsArgs p) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r <= p.n_reads; r += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t g0 = p.off[r];
        if (g0 > p.n_rows) g0 = p.n_rows; // (offsets that do not ascend to n_rows are the caller's fault; no row beyond is looked at)
        p.cons_off[r] = cons_pos_at(p, g0);
    }
}

// kmu_pile_consensus_pos: a query row above n_rows raises info[0], before any output
__global__ void __launch_bounds__(256) k_cons_pos_check(const uint64_t *rows, uint64_t n, uint64_t n_rows, uint32_t *info) {
    bool bad = false;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) bad |= rows[i] > n_rows;
    if (bad) info[0] = 1u;
}
// ... one lane per query
__global__ void __launch_bounds__(256) k_cons_pos(ConsArgs p, const uint64_t *rows, uint64_t n, uint64_t *pos) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t g0 = rows[i];
        pos[i] = cons_pos_at(p, g0 < p.n_rows ? g0 : p.n_rows); // (the check has refused a row above n_rows)
    }
}

} // namespace kmu

using namespace kmu;

// the inputs on the device, the slot index with the refusal of an ins_len that does not belong to n_slots (before any output), the
// count pass and the tile offsets: what kmu_pile_consensus and kmu_pile_consensus_pos share
static int cons_plan(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots, const uint32_t *ins,
                     const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int mem, ConsArgs *out, uint64_t **tile_off_out) {
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    ConsArgs a{};
    uint64_t n_rows = 0;
    KMU_TRY(caller_word(ctx, offsets + n_reads, mem, &n_rows));

    KMU_TRY(stage_to_device(ctx, "cons.pile", pile, (size_t) n_rows * PILE_COLS, mem, &a.pile));
    KMU_TRY(stage_to_device(ctx, "cons.call", call, (size_t) n_rows, mem, &a.call));
    KMU_TRY(stage_to_device(ctx, "cons.len", ins_len, (size_t) n_rows, mem, &a.ins_len));
    KMU_TRY(stage_to_device(ctx, "cons.ins", ins, (size_t) n_slots * CONS_LETTERS, mem, &a.ins));
    a.n_slots = n_slots;
    KMU_TRY(stage_to_device(ctx, "cons.bases", bases, (size_t) n_rows, mem, &a.bases));
    KMU_TRY(stage_to_device(ctx, "cons.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;
    a.n_rows = n_rows;
    a.n_tiles = cons_n_blocks(n_rows);

    // the slot index, and the refusal of an ins_len that does not belong to n_slots: before any output
    uint64_t *slot_off, total_slots = 0;
    KMU_TRY(ins_block_offsets(ctx, "cons.slotoff", a.ins_len, n_rows, &slot_off));
    a.slot_off = slot_off;
    KMU_TRY(read_back(ctx, {{&total_slots, slot_off + a.n_tiles}}));
    if (total_slots != n_slots)
        return refuse(ctx, KMU_E_UNSUPPORTED, "ins_len sums to %llu slots, not to n_slots = %llu", (unsigned long long) total_slots, (unsigned long long) n_slots);

    uint64_t *tile_off;
    KMU_TRY(dev_array(ctx, "cons.tilelen", a.n_tiles ? a.n_tiles : 1, &a.tile_len));
    KMU_TRY(dev_array(ctx, "cons.tileoff", a.n_tiles + 1, &tile_off));
    a.tile_off = tile_off;
    const dim3 grid(grid_for(ctx, a.n_tiles, 4));
    if (a.n_tiles) {
        KMU_TRY(launch(ctx, "k_cons_count", k_cons_tiles<false>, grid, dim3(256), 0, a));
        KMU_TRY(device_scan_u32(ctx, a.tile_len, a.n_tiles, tile_off));
    } else {
        KMU_HIP(ctx, hipMemsetAsync(tile_off, 0, 8, ctx->stream));
    }
    *out = a;
    *tile_off_out = tile_off;
    return KMU_OK;
}

extern "C" int kmu_pile_consensus(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots, const uint32_t *ins,
                                  const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const kmu_consensus_params *p, int mem,
                                  uint64_t *cons_offsets_out, uint8_t *cons_out, uint64_t cap, uint64_t *n_cons_out) {
    if (!ctx || !pile || !call || !ins_len || !bases || !offsets || !p || !cons_offsets_out || !n_cons_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (!ins && n_slots) return fail(ctx, KMU_E_BAD_ARG, "ins is null with n_slots = %llu", (unsigned long long) n_slots);
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    KMU_TRY(check_mem(ctx, mem));
    *n_cons_out = 0;
    ConsArgs a{};
    uint64_t *tile_off, total = 0;
    KMU_TRY(cons_plan(ctx, pile, call, ins_len, n_slots, ins, bases, offsets, n_reads, mem, &a, &tile_off));
    const dim3 grid(grid_for(ctx, a.n_tiles, 4));
    KMU_TRY(place_output(ctx, "cons.consoff", cons_offsets_out, (size_t) n_reads + 1, mem, &a.cons_off));
    KMU_TRY(launch(ctx, "k_cons_offsets", k_cons_offsets, dim3(grid_for(ctx, (uint64_t) n_reads + 1, 256)), dim3(256), 0, a));
    KMU_TRY(bring_output(ctx, cons_offsets_out, a.cons_off, (size_t) n_reads + 1, mem));
    KMU_TRY(read_back(ctx, {{&total, tile_off + a.n_tiles}}));
    *n_cons_out = total;
    if (cons_out && cap < total)
        return refuse(ctx, KMU_E_BAD_ARG, "cap = %llu is below the %llu bytes", (unsigned long long) cap, (unsigned long long) total);
    if (cons_out && total) {
        KMU_TRY(place_output(ctx, "cons.cons", cons_out, total, mem, &a.cons));
        KMU_TRY(launch(ctx, "k_cons_write", k_cons_tiles<true>, grid, dim3(256), 0, a));
        KMU_TRY(bring_output(ctx, cons_out, a.cons, total, mem));
        return finish_sync(ctx);
    }
    return finish_synced(ctx);
}

extern "C" int kmu_pile_consensus_pos(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots, const uint32_t *ins,
                                      const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, const kmu_consensus_params *p, int mem,
                                      const uint64_t *rows, uint64_t n_rows_q, uint64_t *pos_out) {
    if (!ctx || !pile || !call || !ins_len || !bases || !offsets || !p || (n_rows_q && (!rows || !pos_out))) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (!ins && n_slots) return fail(ctx, KMU_E_BAD_ARG, "ins is null with n_slots = %llu", (unsigned long long) n_slots);
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    KMU_TRY(check_mem(ctx, mem));
    ConsArgs a{};
    uint64_t *tile_off;
    KMU_TRY(cons_plan(ctx, pile, call, ins_len, n_slots, ins, bases, offsets, n_reads, mem, &a, &tile_off));
    if (n_rows_q == 0) return finish_synced(ctx);
    const uint64_t *d_rows;
    KMU_TRY(stage_to_device(ctx, "cons.rows", rows, (size_t) n_rows_q, mem, &d_rows));
    uint32_t *info, h_info = 0;
    KMU_TRY(dev_array(ctx, "cons.info", 1, &info));
    KMU_HIP(ctx, hipMemsetAsync(info, 0, 4, ctx->stream));
    const dim3 grid(grid_for(ctx, n_rows_q, 256));
    KMU_TRY(launch(ctx, "k_cons_pos_check", k_cons_pos_check, grid, dim3(256), 0, d_rows, n_rows_q, a.n_rows, info));
    KMU_TRY(read_back(ctx, {{&h_info, info}}));
    if (h_info)
        return refuse(ctx, KMU_E_UNSUPPORTED, "a query row above n_bases = %llu", (unsigned long long) a.n_rows);
    uint64_t *pos;
    KMU_TRY(place_output(ctx, "cons.pos", pos_out, (size_t) n_rows_q, mem, &pos));
    KMU_TRY(launch(ctx, "k_cons_pos", k_cons_pos, grid, dim3(256), 0, a, d_rows, n_rows_q, pos));
    KMU_TRY(bring_output(ctx, pos_out, pos, (size_t) n_rows_q, mem));
    return finish_sync(ctx);
}

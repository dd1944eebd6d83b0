// kmu_chain_pileup.hip -- the read pileup: per-base votes of every chain's CIGAR runs onto both reads (kmu_chain_pileup), and the call
// per base with a summary per read (kmu_pile_call).  The contracts are in include/kmu.h, the index arithmetic in kmu_pile_core.h.
//
//  k_pile_count   one lane per chain: checks the record as kmu_chain_cigar does and the chain's two run offsets, and leaves the
//                 number of tiles (PILE_TILE runs each) of a chain with PATH.  device_scan_u32 turns them into tile offsets.
//  k_pile_starts  one wave per chain: reads the chain's runs a tile at a time, one run per lane, checks every run and sums the bases
//                 of A and of B' the tile consumes; lane 0 leaves (chain, i, j) at the start of every tile.  The sums must end at
//                 (m, n).  Anything wrong raises info[0]: the call is refused at its first synchronisation, before any vote.
//  k_pile_vote    one wave per tile: the lanes scan the tile's run lengths (DPP), leave run start and column scan in LDS, and the
//                 wave walks the tile's columns 64 at a time, one column per lane, so its atomic adds fall on about 64 consecutive
//                 32-byte rows of a table.  The INS / INS_BASES votes of a run come from the lane that owns the run, the ENDS votes
//                 of a chain from lane 0 of its first tile.  Plain uint32 atomicAdd: integer sums commute.
//  k_pile_call    one lane per base: the call byte of its row.
//  k_pile_reads   one wave per read, 64 rows at a time: the summary record.
// The argument checks and the check-and-tile step (k_pile_count, scan, k_pile_starts) are pile_check_inputs and pile_plan of
// kmu_pile_plan.h: kmu_chain_pile_ins (kmu_pile_ins.hip) takes the same inputs and goes through the same two functions.
#include "kmu_ctx.hpp"
#include "kmu_device.h"
#include "kmu_pile_core.h"
#include "kmu_pile_plan.h"

namespace kmu {

static_assert(PILE_OP_I == KMU_CIGAR_I && PILE_OP_D == KMU_CIGAR_D && PILE_OP_EQ == KMU_CIGAR_EQ && PILE_OP_X == KMU_CIGAR_X,
              "the run codes are the header's");
static_assert(PILE_COLS == KMU_PILE_COLS && PILE_DEL == KMU_PILE_DEL && PILE_INS == KMU_PILE_INS && PILE_INS_BASES == KMU_PILE_INS_BASES &&
                  PILE_ENDS == KMU_PILE_ENDS && KMU_PILE_A == 0 && KMU_PILE_T == 3,
              "the columns are the header's");
static_assert(PILE_CALL_NONE == KMU_CALL_NONE && PILE_CALL_INS == KMU_CALL_INS && PILE_CALL_DIFF == KMU_CALL_DIFF, "the call bits are the header's");
static_assert(sizeof(kmu_read_pile) == 32, "kmu_read_pile is 32 bytes");

// the checks of kmu_chain_cigar on a record; beg_*: where the two reads begin
__device__ __forceinline__ bool pile_record_ok(const PileArgs &p, const kmu_chain &rec, uint64_t &beg_a, uint64_t &beg_b) {
    bool ok = rec.read_a < p.n_reads_q && rec.read_b < p.n_reads_db && rec.strand <= 1u && rec.a_start <= rec.a_end && rec.b_start <= rec.b_end;
    beg_a = beg_b = 0;
    if (ok) {
        beg_a = p.off_q[rec.read_a];
        beg_b = p.off_db[rec.read_b];
        ok = rec.a_end <= p.off_q[rec.read_a + 1u] - beg_a && rec.b_end <= p.off_db[rec.read_b + 1u] - beg_b;
    }
    return ok;
}

__global__ void __launch_bounds__(256) k_pile_count(PileArgs p) {
    for (uint64_t c = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; c < p.n_chains; c += (uint64_t) gridDim.x * blockDim.x) {
        const kmu_chain rec = p.chains[c];
        const uint64_t lo = p.op_off[c], hi = p.op_off[c + 1];
        uint64_t beg_a, beg_b, tiles = 0;
        bool ok = pile_record_ok(p, rec, beg_a, beg_b) && lo <= hi && hi <= p.n_ops;
        if (ok) {
            if (p.aln[c].flags & KMU_ALN_PATH) tiles = pile_n_tiles(hi - lo);
            else ok = lo == hi;
        }
        if (!ok || tiles > 0xFFFFFFFFull) {
            p.info[0] = 1u;
            tiles = 0;
        }
        p.n_tiles[c] = (uint32_t) tiles;
    }
}

__global__ void __launch_bounds__(64) k_pile_starts(PileArgs p) {
    const uint32_t lane = (uint32_t) lane_id();
    bool bad = false;
    for (uint64_t c = blockIdx.x; c < p.n_chains; c += gridDim.x) {
        if (!(p.aln[c].flags & KMU_ALN_PATH)) continue; // (k_pile_count has seen that it has no runs)
        const kmu_chain rec = p.chains[c];
        const uint64_t lo = p.op_off[c], hi = p.op_off[c + 1], t0 = p.tile_off[c];
        if (!(rec.a_start <= rec.a_end && rec.b_start <= rec.b_end && lo <= hi && hi <= p.n_ops) || p.tile_off[c + 1] - t0 != pile_n_tiles(hi - lo)) {
            bad = true; // (k_pile_count has refused it)
            continue;
        }
        const uint64_t m = rec.a_end - rec.a_start, n = rec.b_end - rec.b_start;
        uint64_t i = 0, j = 0;
        for (uint64_t r0 = lo, t = t0; r0 < hi; r0 += PILE_TILE, t++) {
            uint32_t da = 0, db = 0;
            const bool ok = r0 + lane >= hi || pile_run_adv(p.ops[r0 + lane], da, db);
            if (lane == 0 && t < p.tile_cap) p.tiles[t] = PileTileRec{c, (uint32_t) i, (uint32_t) j};
            i += wave_sum_u64(da);
            j += wave_sum_u64(db);
            if (__any(!ok) || i > m || j > n) { // (uniform; before the sums can pass 2^32: a tile adds less than 2^34)
                i = ~0ull;
                break;
            }
        }
        if (i != m || j != n) bad = true;
    }
    if (bad) p.info[0] = 1u;
}

__global__ void __launch_bounds__(64) k_pile_vote(PileArgs p, uint64_t n_tiles) {
    __shared__ uint64_t s_incl[PILE_TILE];
    __shared__ uint32_t s_run[PILE_TILE], s_i0[PILE_TILE], s_j0[PILE_TILE];
    const uint32_t lane = (uint32_t) lane_id();
    const bool side_q = (p.flags & KMU_PILE_Q) != 0, side_db = (p.flags & KMU_PILE_DB) != 0;
    uint32_t non_acgt = 0;
    for (uint64_t t = blockIdx.x; t < n_tiles; t += gridDim.x) {
        const PileTileRec tr = p.tiles[t];
        const kmu_chain rec = p.chains[tr.chain];
        const uint64_t first = p.op_off[tr.chain] + (t - p.tile_off[tr.chain]) * PILE_TILE, hi = p.op_off[tr.chain + 1];
        const uint32_t nr = hi - first < PILE_TILE ? (uint32_t) (hi - first) : PILE_TILE;
        const uint32_t m = rec.a_end - rec.a_start, n = rec.b_end - rec.b_start;
        uint32_t *const row_q = p.pile_q + (p.off_q[rec.read_a] + rec.a_start) * PILE_COLS;   // row of A's base 0 (used where side_q)
        uint32_t *const row_db = p.pile_db + p.off_db[rec.read_b] * PILE_COLS;                // row of read b's base 0 (where side_db)
        const uint8_t *const let_a = p.bases_q + p.off_q[rec.read_a] + rec.a_start, *const let_b = p.bases_db + p.off_db[rec.read_b];

        // the tile's runs: one per lane; where each begins, and the scan of the columns
        uint32_t run = 0, da = 0, db = 0;
        if (lane < nr) {
            run = p.ops[first + lane];
            pile_run_adv(run, da, db);
        }
        const uint32_t op = run & 15u, len = run >> 4;
        const uint32_t ia = wave_incl_scan_u32(da), ib = wave_incl_scan_u32(db); // (the chain's sums are m and n: below 2^32)
        const uint32_t i0 = tr.i + ia - da, j0 = tr.j + ib - db;
        const uint64_t incl = (uint64_t) ia + wave_incl_scan_u32(len - da); // columns: the bases of A, and the bases of D runs
        __syncthreads(); // the reads of the tile before are done
        s_incl[lane] = incl;
        s_run[lane] = run;
        s_i0[lane] = i0;
        s_j0[lane] = j0;
        __syncthreads();
        const uint64_t total = s_incl[PILE_TILE - 1u];

        // the votes of a run as a whole, and the ends of the chain
        if (lane < nr) {
            const uint32_t ra = pile_run_row_a(op, i0), rb = pile_run_row_b(op, rec.strand, j0, n);
            if (side_q && ra != PILE_NONE && ra < m) {
                atomicAdd(row_q + (uint64_t) ra * PILE_COLS + PILE_INS, 1u);
                atomicAdd(row_q + (uint64_t) ra * PILE_COLS + PILE_INS_BASES, len);
            }
            if (side_db && rb != PILE_NONE && rb < n) {
                uint32_t *row = row_db + (uint64_t) pile_b_pos(rec.strand, rec.b_start, rec.b_end, rb) * PILE_COLS;
                atomicAdd(row + PILE_INS, 1u);
                atomicAdd(row + PILE_INS_BASES, len);
            }
        }
        if (lane == 0 && t == p.tile_off[tr.chain]) {
            if (side_q && m) {
                atomicAdd(row_q + PILE_ENDS, 1u);
                atomicAdd(row_q + (uint64_t) (m - 1u) * PILE_COLS + PILE_ENDS, 1u);
            }
            if (side_db && n) {
                atomicAdd(row_db + (uint64_t) rec.b_start * PILE_COLS + PILE_ENDS, 1u);
                atomicAdd(row_db + (uint64_t) (rec.b_end - 1u) * PILE_COLS + PILE_ENDS, 1u);
            }
        }

        // the columns: one per lane
        for (uint64_t col = lane; col < total; col += PILE_TILE) {
            const uint32_t r = pile_find_run(s_incl, nr, col);
            const uint32_t rop = s_run[r] & 15u;
            const PileCol pc = pile_column(rop, s_i0[r], s_j0[r], (uint32_t) (col - (r ? s_incl[r - 1u] : 0ull)));
            const bool has_a = pc.i != PILE_NONE, has_b = pc.j != PILE_NONE;
            if ((has_a && pc.i >= m) || (has_b && pc.j >= n)) continue; // (k_pile_starts has checked the sums: never taken)
            const uint32_t pos_b = has_b ? pile_b_pos(rec.strand, rec.b_start, rec.b_end, pc.j) : 0u;
            if (side_q && has_a) {
                uint32_t code = PILE_DEL;
                if (has_b) {
                    code = pile_code(let_b[pos_b]);
                    if (code == PILE_NO_CODE) non_acgt = 1u;
                    else if (rec.strand) code = 3u - code;
                }
                if (code != PILE_NO_CODE) atomicAdd(row_q + (uint64_t) pc.i * PILE_COLS + code, 1u);
            }
            if (side_db && has_b) {
                uint32_t code = PILE_DEL;
                if (has_a) {
                    code = pile_code(let_a[pc.i]);
                    if (code == PILE_NO_CODE) non_acgt = 1u;
                    else if (rec.strand) code = 3u - code;
                }
                if (code != PILE_NO_CODE) atomicAdd(row_db + (uint64_t) pos_b * PILE_COLS + code, 1u);
            }
        }
    }
    if (non_acgt) p.info[1] = 1u;
}

struct PileCallArgs {
    const uint32_t *pile;
    const uint8_t *bases;
    const uint64_t *off;
    uint32_t n_reads;
    uint32_t min_depth;
    uint8_t *call;
    kmu_read_pile *reads;
};

__global__ void __launch_bounds__(256) k_pile_call(PileCallArgs p) {
    const uint64_t n_bases = p.off[p.n_reads];
    for (uint64_t g = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; g < n_bases; g += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t row[PILE_COLS];
        for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = p.pile[g * PILE_COLS + k];
        uint64_t depth;
        p.call[g] = (uint8_t) pile_call_row(row, p.bases[g], p.min_depth, depth);
    }
}

__global__ void __launch_bounds__(256) k_pile_reads(PileCallArgs p) {
    const uint32_t lane = (uint32_t) lane_id();
    for (uint64_t r = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); r < p.n_reads; r += (uint64_t) gridDim.x * 4u) {
        const uint64_t beg = p.off[r], end = p.off[r + 1];
        uint32_t covered = 0, n_diff = 0, n_del = 0, n_ins = 0, max_depth = 0;
        uint64_t depth_sum = 0;
        for (uint64_t g = beg + lane; g < end; g += 64u) {
            uint32_t row[PILE_COLS];
            for (uint32_t k = 0; k < PILE_COLS; k++) row[k] = p.pile[g * PILE_COLS + k];
            uint64_t depth;
            const uint32_t call = pile_call_row(row, p.bases[g], p.min_depth, depth);
            const uint32_t d32 = depth > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) depth;
            depth_sum += depth;
            max_depth = d32 > max_depth ? d32 : max_depth;
            if ((call & 7u) != PILE_CALL_NONE) {
                covered++;
                n_diff += (call & PILE_CALL_DIFF) != 0u;
                n_del += (call & 7u) == PILE_DEL;
                n_ins += (call & PILE_CALL_INS) != 0u;
            }
        }
        kmu_read_pile o;
        o.n_bases = (uint32_t) (end - beg);
        o.covered = wave_sum_u32(covered);
        o.n_diff = wave_sum_u32(n_diff);
        o.n_del = wave_sum_u32(n_del);
        o.n_ins = wave_sum_u32(n_ins);
        o.max_depth = wave_max_u32(max_depth);
        o.depth_sum = wave_sum_u64(depth_sum);
        if (lane == 0) p.reads[r] = o;
    }
}

} // namespace kmu

using namespace kmu;

namespace kmu {

int pile_check_inputs(kmu_ctx *ctx, const PileInputs &in, const void *table_q, const void *table_db) {
    if (!ctx || !in.chains || !in.aln || !in.op_offsets || !in.bases_q || !in.offsets_q || !in.bases_db || !in.offsets_db || !in.p)
        return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (!in.ops && in.n_ops) return fail(ctx, KMU_E_BAD_ARG, "ops is null with n_ops = %llu", (unsigned long long) in.n_ops);
    const uint32_t flags = in.p->flags;
    if (!flags || (flags & ~(KMU_PILE_Q | KMU_PILE_DB))) return fail(ctx, KMU_E_BAD_ARG, "flags 0x%x: KMU_PILE_Q, KMU_PILE_DB or both", flags);
    const bool side_q = flags & KMU_PILE_Q, side_db = flags & KMU_PILE_DB;
    if ((side_q && !table_q) || (side_db && !table_db)) return fail(ctx, KMU_E_BAD_ARG, "null table for a side that is asked for");
    KMU_TRY(check_mem(ctx, in.mem));
    if (side_q && side_db && table_q == table_db && !in.self())
        return fail(ctx, KMU_E_BAD_ARG, "one table for both sides needs the two batches to be the same arrays");
    if (in.n_chains && (in.n_reads_q == 0 || in.n_reads_db == 0)) return fail(ctx, KMU_E_BAD_ARG, "chains but no reads");
    return KMU_OK;
}

int pile_plan(kmu_ctx *ctx, const PileInputs &in, PileArgs *out, uint64_t *n_tiles_out) {
    const int mem = in.mem;
    const uint64_t n_chains = in.n_chains;
    PileArgs a{};
    KMU_TRY(stage_to_device(ctx, "pile.chains", in.chains, (size_t) n_chains, mem, &a.chains));
    a.n_chains = n_chains;
    KMU_TRY(stage_to_device(ctx, "pile.aln", in.aln, (size_t) n_chains, mem, &a.aln));
    KMU_TRY(stage_to_device(ctx, "pile.opoff", in.op_offsets, (size_t) (n_chains + 1), mem, &a.op_off));
    KMU_TRY(stage_to_device(ctx, "pile.ops", in.ops, (size_t) in.n_ops, mem, &a.ops));
    a.n_ops = in.n_ops;
    KMU_TRY(stage_to_device(ctx, "pile.basesq", in.bases_q, mem == KMU_MEM_HOST ? (size_t) in.offsets_q[in.n_reads_q] : 0, mem, &a.bases_q));
    KMU_TRY(stage_to_device(ctx, "pile.offq", in.offsets_q, (size_t) in.n_reads_q + 1, mem, &a.off_q));
    if (in.self()) { // a self-join is staged once
        a.bases_db = a.bases_q;
        a.off_db = a.off_q;
    } else {
        KMU_TRY(stage_to_device(ctx, "pile.basesdb", in.bases_db, mem == KMU_MEM_HOST ? (size_t) in.offsets_db[in.n_reads_db] : 0, mem, &a.bases_db));
        KMU_TRY(stage_to_device(ctx, "pile.offdb", in.offsets_db, (size_t) in.n_reads_db + 1, mem, &a.off_db));
    }
    a.n_reads_q = in.n_reads_q;
    a.n_reads_db = in.n_reads_db;
    a.flags = in.p->flags;
    uint64_t *d_tile_off;
    a.tile_cap = in.n_ops / PILE_TILE + n_chains; // every chain's tiles, when the offsets are what they must be
    KMU_TRY(dev_array(ctx, "pile.info", 2, &a.info));
    KMU_TRY(dev_array(ctx, "pile.ntiles", n_chains, &a.n_tiles));
    KMU_TRY(dev_array(ctx, "pile.tileoff", n_chains + 1, &d_tile_off));
    KMU_TRY(dev_array(ctx, "pile.tiles", a.tile_cap, &a.tiles));
    a.tile_off = d_tile_off;
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, 8, ctx->stream));

    KMU_TRY(launch(ctx, "k_pile_count", k_pile_count, dim3(grid_for(ctx, n_chains, 256)), dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.n_tiles, n_chains, d_tile_off));
    KMU_TRY(launch(ctx, "k_pile_starts", k_pile_starts, dim3(grid_for(ctx, n_chains, 1, 16)), dim3(64), 0, a));
    uint32_t h_info[2] = {0, 0};
    uint64_t n_tiles = 0;
    KMU_TRY(read_back(ctx, {{h_info, a.info, sizeof h_info}, {&n_tiles, d_tile_off + n_chains}}));
    if (h_info[0] || n_tiles > a.tile_cap)
        return refuse(ctx, KMU_E_UNSUPPORTED, "a chain record kmu_chain_cigar would refuse, run offsets that decrease or end above n_ops, runs on a chain "
                                              "without PATH, a run with an unknown op or of length 0, or runs that do not sum to the chain's segments");
    *out = a;
    *n_tiles_out = n_tiles;
    return KMU_OK;
}

} // namespace kmu

extern "C" int kmu_chain_pileup(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln, const uint64_t *op_offsets,
                                const uint32_t *ops, uint64_t n_ops, const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                                const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db, const kmu_pileup_params *p, int mem,
                                uint32_t *pile_q, uint32_t *pile_db) {
    const PileInputs in{chains, n_chains, aln, op_offsets, ops, n_ops, bases_q, offsets_q, n_reads_q, bases_db, offsets_db, n_reads_db, p, mem};
    KMU_TRY(pile_check_inputs(ctx, in, pile_q, pile_db));
    const bool side_q = p->flags & KMU_PILE_Q, side_db = p->flags & KMU_PILE_DB;
    const bool shared = side_q && side_db && pile_q == pile_db;
    if (n_chains == 0) return KMU_OK;
    KMU_HIP(ctx, hipSetDevice(ctx->device));

    PileArgs a{};
    uint64_t n_tiles = 0;
    KMU_TRY(pile_plan(ctx, in, &a, &n_tiles));
    a.pile_q = side_q ? pile_q : nullptr;
    a.pile_db = side_db ? pile_db : nullptr;
    const size_t words_q = mem == KMU_MEM_HOST && side_q ? (size_t) offsets_q[n_reads_q] * PILE_COLS : 0;
    const size_t words_db = mem == KMU_MEM_HOST && side_db && !shared ? (size_t) offsets_db[n_reads_db] * PILE_COLS : 0;
    if (mem == KMU_MEM_HOST) { // the votes of this call alone, added to the caller's tables at the end
        if (side_q) {
            KMU_TRY(dev_array(ctx, "pile.tableq", words_q ? words_q : 1, &a.pile_q));
            KMU_HIP(ctx, hipMemsetAsync(a.pile_q, 0, words_q * 4, ctx->stream));
        }
        if (shared) a.pile_db = a.pile_q;
        else if (side_db) {
            KMU_TRY(dev_array(ctx, "pile.tabledb", words_db ? words_db : 1, &a.pile_db));
            KMU_HIP(ctx, hipMemsetAsync(a.pile_db, 0, words_db * 4, ctx->stream));
        }
    }
    uint32_t h_info[2] = {0, 0};
    if (n_tiles) KMU_TRY(launch(ctx, "k_pile_vote", k_pile_vote, dim3(grid_for(ctx, n_tiles, 1, 32)), dim3(64), 0, a, n_tiles));
    KMU_TRY(read_back(ctx, {{h_info, a.info, sizeof h_info}}));
    KMU_TRY(finish_synced(ctx));
    std::vector<uint32_t> got;
    auto add_down = [&](uint32_t *mine, const uint32_t *dev, size_t words) -> int { // the caller's table += this call's
        got.resize(words);
        if (words) KMU_HIP(ctx, hipMemcpy(got.data(), dev, words * 4, hipMemcpyDeviceToHost));
        for (size_t k = 0; k < words; k++) mine[k] += got[k];
        return KMU_OK;
    };
    if (mem == KMU_MEM_HOST) {
        if (side_q) KMU_TRY(add_down(pile_q, a.pile_q, words_q));
        if (side_db && !shared) KMU_TRY(add_down(pile_db, a.pile_db, words_db));
    }
    if (h_info[1]) return fail(ctx, KMU_E_NON_ACGT, "a voted letter outside ACGTacgt");
    return KMU_OK;
}

extern "C" int kmu_pile_call(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                             const kmu_pile_call_params *p, int mem, uint8_t *call_out, kmu_read_pile *reads_out) {
    if (!ctx || !pile || !bases || !offsets || !p || (!call_out && !reads_out)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (p->min_depth == 0) return fail(ctx, KMU_E_BAD_ARG, "min_depth must be at least 1");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    KMU_TRY(check_mem(ctx, mem));
    if (n_reads == 0) return KMU_OK;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t n_bases = 0;
    KMU_TRY(caller_word(ctx, offsets + n_reads, mem, &n_bases)); // (the grid)

    PileCallArgs a{};
    KMU_TRY(stage_to_device(ctx, "pcall.pile", pile, (size_t) n_bases * PILE_COLS, mem, &a.pile));
    KMU_TRY(stage_to_device(ctx, "pcall.bases", bases, (size_t) n_bases, mem, &a.bases));
    KMU_TRY(stage_to_device(ctx, "pcall.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;
    a.min_depth = p->min_depth;
    KMU_TRY(place_output(ctx, "pcall.call", call_out, n_bases ? n_bases : 1, mem, &a.call));
    KMU_TRY(place_output(ctx, "pcall.reads", reads_out, n_reads, mem, &a.reads));
    if (call_out && n_bases) KMU_TRY(launch(ctx, "k_pile_call", k_pile_call, dim3(grid_for(ctx, n_bases, 256)), dim3(256), 0, a));
    if (reads_out) KMU_TRY(launch(ctx, "k_pile_reads", k_pile_reads, dim3(grid_for(ctx, n_reads, 4)), dim3(256), 0, a));
    if (n_bases) KMU_TRY(bring_output(ctx, call_out, a.call, n_bases, mem));
    KMU_TRY(bring_output(ctx, reads_out, a.reads, n_reads, mem));
    return finish_sync(ctx);
}

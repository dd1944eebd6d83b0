// kmu_syncmers.hip -- closed and open syncmers: the k-mers of every read whose smallest s-mer sits at offset t or u - t, u = k - s
// (kmu_read_syncmers; include/kmu.h has the rules).
//
// The k-mer positions of a read are cut into tiles of KMU_SYNCMER_TILE; a read with nk k-mers has ceil(nk / TILE) tiles, a read
// without k-mers none.  The scheme is that of kmu_minimizers.hip, and the two steps that are the same are the same code:
//  k_mini_tiles      (kmu_seed_tiles.h, with w = 1: a window is a k-mer) tiles per read, and the bytes of reads shorter than k.
//  k_read_syncmers   one wave (a 64-thread workgroup) per tile, tiles dealt grid-stride; tile -> read by wave_find_read over
//                    tile_off.  The tile with k-mer positions [j0, j1) hashes the s-mers [j0, j1 + u) into LDS with SeqView +
//                    wave_step_kmers + apply_fhash under the s-mers' KmerCfg: they cover every base of the tile's k-mers, so
//                    every base is validated, and j1 + u <= nk + u is the read's number of s-mers, so nothing is clipped.  No
//                    position in front of the tile is needed: a verdict depends on its own u + 1 entries only.
//                    Sliding minimum VALUE over u + 1 <= 32 entries: every lane keeps the state of its entries e = c * 64 + lane
//                    in registers; a doubling pass d = 1, 2, 4, ... takes min(own, state of entry e + d), so that after log2(D)
//                    passes (D the largest power of two <= u + 1) an entry is the minimum of [e, e + D); m is min(entry e, entry
//                    e + u + 1 - D).  The first pass reads the hashes themselves; the later ones publish the state in a second
//                    LDS array, because the hashes are needed once more: k-mer e is selected iff g(e + t) == m or g(e + u - t)
//                    == m.  No position and no tie rule take part.  Selected positions are ranked by ballots in position order.
//                    COUNT leaves the number per tile and ends there: it hashes s-mers only.  WRITE leaves every ballot and the
//                    count in front of it in LDS, then walks the tile's k-mers with wave_step_kmers under k; a position looks up
//                    its bit and only a selected one pays apply_fhash (k rotations under ntHash) and stores hash / position /
//                    read / strand at its rank.
//  k_mini_offsets    (kmu_seed_tiles.h) sync_offsets[i] = the offset of read i's first tile.
//  LDS: 8.5 KiB hashes + 8.5 KiB state + 192 B ballots and ranks = 17.2 KiB per one-wave workgroup (nine per CU).
#include <algorithm>

#include "kmu_ctx.hpp"
#include "kmu_flat.h"
#include "kmu_seed_tiles.h"
#include "kmu_stream.h"

namespace kmu {

static constexpr uint32_t SYNC_T = KMU_SYNCMER_TILE;
static constexpr uint32_t SYNC_MAX_U = 63;                 // k <= 32 today; the entries behind a tile fit one more chunk
static constexpr uint32_t SYNC_NE = SYNC_T + 64;           // s-mers a tile holds at most: TILE + u, dealt to 64 lanes
static constexpr uint32_t SYNC_CH = SYNC_NE / 64;          // ... per lane
static constexpr uint32_t SYNC_PC = SYNC_T / 64;           // ballots per tile
static_assert(SYNC_T % 64 == 0 && SYNC_T + SYNC_MAX_U <= SYNC_NE, "a tile's s-mers fit its LDS arrays");

struct SyncArgs {
    const uint8_t *bases;
    const uint64_t *offsets;  // n_seq + 1
    const uint64_t *tile_off; // n_seq + 1: first tile of every read
    uint32_t n_seq;
    uint32_t t;
    uint64_t total_bytes;     // size of `bases`, or 0: offsets[n_seq]
    uint64_t room;            // COUNT: entries of `counts` (those behind the last tile are zeroed); WRITE: the number of tiles
    KmerCfg cfg;              // the k-mers: what is written
    KmerCfg scfg;             // the s-mers: what orders
    uint32_t *counts;         // COUNT: selected k-mers per tile
    const uint64_t *coff;     // WRITE: first entry of every tile
    uint64_t *hashes;
    uint32_t *pos, *read;     // may be null
    uint8_t *strand;          // may be null
    uint32_t *err;
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_read_syncmers(SyncArgs a) {
    __shared__ uint64_t keys[SYNC_NE];  // g of the tile's s-mers
    __shared__ uint64_t state[SYNC_NE]; // the running minima between two passes
    __shared__ uint64_t selw[SYNC_PC];  // WRITE: the ballot of every 64 positions
    __shared__ uint32_t pre[SYNC_PC];   // ... and the number selected in front of it
    const uint32_t lane = (uint32_t) lane_id();
    const int k = a.cfg.k, s = a.scfg.k;
    const uint32_t u = (uint32_t) (k - s), off_a = a.t, off_b = u - a.t;
    const uint64_t total = a.total_bytes ? a.total_bytes : a.offsets[a.n_seq];
    const uint64_t n_tiles = a.tile_off[a.n_seq];
    const bool canon = a.cfg.fhash == KMU_FHASH_CANON_RAW || a.cfg.fhash == KMU_FHASH_CANON_VALUE || a.cfg.fhash == KMU_FHASH_CANON_INVHASH;
    uint32_t D = 1; // the largest power of two <= u + 1
    while (D * 2 <= u + 1) D *= 2;
    const uint32_t tail = u + 1 - D;
    uint32_t bad = 0;
    for (uint64_t t = blockIdx.x; t < a.room; t += gridDim.x) {
        if (t >= n_tiles) { // (COUNT only: the counts array may be longer than the tiles)
            if (!WRITE && lane == 0) a.counts[t] = 0u;
            continue;
        }
        const uint32_t r = wave_find_read(a.tile_off, a.n_seq, t);
        const uint64_t rbeg = a.offsets[r], L = a.offsets[r + 1] - rbeg;
        const uint64_t nk = L - (uint64_t) k + 1; // > 0: the read has a tile
        const uint64_t j0 = (t - a.tile_off[r]) * SYNC_T, j1 = std::min<uint64_t>(j0 + SYNC_T, nk);
        const uint32_t n_pos = (uint32_t) (j1 - j0);  // k-mers of the tile, <= TILE
        const uint32_t n_real = n_pos + u;            // s-mers of the tile, <= TILE + u
        const uint32_t nch = (n_real + 63) / 64, npc = (n_pos + 63) / 64;
        SeqView sv;
        sv.base = a.bases; sv.begin = rbeg; sv.len = L; sv.total = total; sv.packed = 0;
        const uint64_t lead = seq_lead(sv);
        for (uint64_t st = (j0 + lead) / 1024; st <= (j0 + n_real - 1 + lead) / 1024; st++)
            bad |= wave_step_kmers(sv, s, st, j0, j0 + n_real, [&](uint64_t p, uint64_t val, uint64_t rc) {
                keys[(uint32_t) (p - j0)] = apply_fhash(a.scfg, val, rc);
            });
        __syncthreads();
        uint64_t h[SYNC_CH];
#pragma unroll
        for (uint32_t c = 0; c < SYNC_CH; c++) {
            const uint32_t e = c * 64 + lane;
            h[c] = c < nch && e < n_real ? keys[e] : 0xFFFFFFFFFFFFFFFFull;
        }
        // min(own, state of entry e + d); the first pass finds the state of the entries in `keys`, which stays as it is
        bool first = true;
        auto combine = [&](uint32_t d) {
            const uint64_t *src = keys;
            if (!first) {
#pragma unroll
                for (uint32_t c = 0; c < SYNC_CH; c++)
                    if (c < nch) state[c * 64 + lane] = h[c];
                __syncthreads();
                src = state;
            }
#pragma unroll
            for (uint32_t c = 0; c < SYNC_CH; c++)
                if (c < nch) {
                    const uint32_t e2 = c * 64 + lane + d;
                    if (e2 < n_real) h[c] = std::min(h[c], src[e2]);
                }
            __syncthreads();
            first = false;
        };
        for (uint32_t d = 1; d < D; d <<= 1) combine(d);
        if (tail) combine(tail);
        uint32_t run = 0;
#pragma unroll
        for (uint32_t c = 0; c < SYNC_PC; c++)
            if (c < npc) {
                const uint32_t e = c * 64 + lane;
                const bool sel = e < n_pos && (keys[e + off_a] == h[c] || keys[e + off_b] == h[c]);
                const uint64_t bal = __ballot(sel);
                if (WRITE && lane == 0) {
                    selw[c] = bal;
                    pre[c] = run;
                }
                run += (uint32_t) __popcll(bal);
            }
        if (!WRITE && lane == 0) a.counts[t] = run;
        if (WRITE) {
            __syncthreads();
            const uint64_t at = a.coff[t];
            for (uint64_t st = (j0 + lead) / 1024; st <= (j1 - 1 + lead) / 1024; st++)
                bad |= wave_step_kmers(sv, k, st, j0, j1, [&](uint64_t p, uint64_t val, uint64_t rc) {
                    const uint32_t e = (uint32_t) (p - j0);
                    const uint64_t word = selw[e >> 6], bit = 1ull << (e & 63u);
                    if (word & bit) {
                        const uint64_t idx = at + pre[e >> 6] + (uint32_t) __popcll(word & (bit - 1ull));
                        a.hashes[idx] = apply_fhash(a.cfg, val, rc);
                        if (a.pos) a.pos[idx] = (uint32_t) p;
                        if (a.read) a.read[idx] = r;
                        if (a.strand) a.strand[idx] = (uint8_t) (canon && rc < val);
                    }
                });
        }
        __syncthreads(); // the next tile overwrites the LDS arrays
    }
    if (bad) atomicOr(a.err, DERR_NON_ACGT);
}

} // namespace kmu

using namespace kmu;

static bool sync_fhash_is_nthash(int fhash) { return fhash == KMU_FHASH_CANON_NTHASH || fhash == KMU_FHASH_CANON_NTHASH_8B; }

extern "C" int kmu_read_syncmers(kmu_ctx *ctx, const kmu_hash_params *p, const kmu_syncmer_params *sp, const uint8_t *bases,
                                 const uint64_t *offsets, uint32_t n_seq, uint64_t *hashes_out, uint32_t *pos_out, uint32_t *read_out,
                                 uint8_t *strand_out, uint64_t cap, uint64_t *sync_offsets_out, uint64_t *n_out) {
    if (!ctx || !p || !sp || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null ctx, params, syncmer params or n_out");
    *n_out = 0;
    const int mem = p->mem;
    KMU_TRY(check_mem(ctx, mem));
    if (kmer_is_aa(p->kmer_type) || kmer_is_aa(sp->s_kmer_type)) return fail(ctx, KMU_E_BAD_ALPHABET, "syncmers are defined on DNA k-mers");
    if (p->input_kind == KMU_INPUT_PACKED2) return fail(ctx, KMU_E_UNSUPPORTED, "syncmers take unpacked (ASCII) bases");
    KMU_TRY(check_hash_params(ctx, p));
    if (sp->s <= 0 || sp->s > p->kmer_size) return fail(ctx, KMU_E_BAD_ARG, "syncmers need 1 <= s <= k: s = %d, k = %d", sp->s, p->kmer_size);
    kmu_hash_params shp = *p; // the s-mers as kmu_kmer_hashes would be asked for them
    shp.kmer_type = sp->s_kmer_type;
    shp.kmer_size = sp->s;
    shp.fhash = sp->s_fhash;
    KMU_TRY(check_hash_params(ctx, &shp));
    const uint32_t k = (uint32_t) p->kmer_size, u = k - (uint32_t) sp->s;
    if (sp->t > u / 2) return fail(ctx, KMU_E_BAD_ARG, "syncmers need t <= (k - s) / 2 = %u: t = %u", u / 2, sp->t);
    if (u > SYNC_MAX_U) return fail(ctx, KMU_E_UNSUPPORTED, "k - s = %u above %u", u, SYNC_MAX_U);
    if (strand_out && sync_fhash_is_nthash(p->fhash))
        return fail(ctx, KMU_E_UNSUPPORTED, "the canonical ntHash does not expose its strand: pass strand_out = NULL");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_seq == 0) {
        KMU_TRY(zero_first_offset(ctx, sync_offsets_out, mem));
        return finish_call(ctx, mem);
    }
    if (!offsets || !bases) return fail(ctx, KMU_E_BAD_ARG, "null sequence buffers");
    // the number of tiles sizes the per-tile workspace.  Host arrays: counted here, with the length check.  Device arrays: the
    // workspace as large as it already is; the count below is done again if the tiles did not fit.
    uint64_t room = 0;
    if (mem == KMU_MEM_HOST) {
        for (uint32_t i = 0; i < n_seq; i++) {
            const uint64_t L = offsets[i + 1] - offsets[i];
            if (L > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "read %u has %llu bases: positions are uint32", i, (unsigned long long) L);
            room += (mini_windows(L, k, 1) + SYNC_T - 1) / SYNC_T;
        }
        room = std::max<uint64_t>(room, 1);
    } else {
        room = std::max<uint64_t>(ctx->bufs["sync.counts"].bytes / 4, 1u << 16);
    }
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, mem, &ds));
    SyncArgs a{};
    a.bases = ds.bases;
    a.offsets = ds.offsets;
    a.n_seq = n_seq;
    a.t = sp->t;
    a.total_bytes = ds.total_bytes;
    a.cfg = KmerCfg{p->kmer_type, p->kmer_size, p->fhash};
    a.scfg = KmerCfg{sp->s_kmer_type, sp->s, sp->s_fhash};
    KMU_TRY(get_err_word(ctx, &a.err));
    uint32_t *ntiles;
    uint64_t *tile_off;
    KMU_TRY(dev_array(ctx, "sync.ntiles", (size_t) n_seq + 1, &ntiles));
    KMU_TRY(dev_array(ctx, "sync.tile_off", (size_t) n_seq + 1, &tile_off));
    KMU_TRY(launch(ctx, nullptr, k_mini_tiles, dim3(grid_for(ctx, n_seq, 256)), dim3(256), 0, ds.bases, ds.offsets, n_seq, k, 1u, ntiles, a.err));
    KMU_TRY(device_scan_u32(ctx, ntiles, n_seq, tile_off));
    a.tile_off = tile_off;

    // COUNT, offsets, total
    uint64_t *coff = nullptr;
    uint64_t head[2] = {0, 0}; // tiles, syncmers
    for (;;) {
        if (room > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu tiles of k-mers: 2^32 or more", (unsigned long long) room);
        KMU_TRY(dev_array(ctx, "sync.counts", (size_t) room, &a.counts));
        KMU_TRY(dev_array(ctx, "sync.coff", (size_t) room + 1, &coff));
        a.room = room;
        const uint32_t grid = (uint32_t) std::min<uint64_t>(room, (uint64_t) ctx->num_cus * 40);
        KMU_TRY(launch(ctx, "k_read_syncmers_count", k_read_syncmers<false>, dim3(grid), dim3(64), 0, a));
        KMU_TRY(device_scan_u32(ctx, a.counts, room, coff));
        KMU_TRY(read_back(ctx, {{&head[0], tile_off + n_seq}, {&head[1], coff + room}}));
        if (head[0] <= room) break;
        room = head[0]; // (device arrays, more tiles than the workspace had room for)
    }
    const uint64_t n_tiles = head[0], total = head[1];
    *n_out = total;
    uint64_t *d_soff;
    KMU_TRY(place_output(ctx, "sync.soff", sync_offsets_out, (size_t) n_seq + 1, mem, &d_soff));
    if (sync_offsets_out) {
        KMU_TRY(launch(ctx, nullptr, k_mini_offsets, dim3(grid_for(ctx, (uint64_t) n_seq + 1, 256)), dim3(256), 0, tile_off, coff, n_seq, d_soff));
        KMU_TRY(bring_output(ctx, sync_offsets_out, d_soff, (size_t) n_seq + 1, mem));
    }
    if (!hashes_out || total == 0) return finish_checked(ctx, mem, a.err);
    if (cap < total) {
        KMU_TRY(finish_checked(ctx, mem, a.err));
        return fail(ctx, KMU_E_BAD_ARG, "%llu syncmers, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.room = n_tiles;
    a.coff = coff;
    KMU_TRY(place_output(ctx, "sync.hashes", hashes_out, (size_t) total, mem, &a.hashes));
    KMU_TRY(place_output(ctx, "sync.pos", pos_out, (size_t) total, mem, &a.pos));
    KMU_TRY(place_output(ctx, "sync.read", read_out, (size_t) total, mem, &a.read));
    KMU_TRY(place_output(ctx, "sync.strand", strand_out, (size_t) total, mem, &a.strand));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(n_tiles, (uint64_t) ctx->num_cus * 40);
    KMU_TRY(launch(ctx, "k_read_syncmers_write", k_read_syncmers<true>, dim3(grid), dim3(64), 0, a));
    KMU_TRY(bring_output(ctx, hashes_out, a.hashes, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, pos_out, a.pos, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, read_out, a.read, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, strand_out, a.strand, (size_t) total, mem));
    return finish_checked(ctx, mem, a.err);
}

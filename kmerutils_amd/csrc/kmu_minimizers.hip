// kmu_minimizers.hip -- window minimizers: the k-mer of smallest hash in every run of w consecutive k-mers of every read, ties to
// the smallest position, each chosen position once (kmu_minimizer_layout / kmu_read_minimizers; include/kmu.h has the rules).
//
// The windows of a read are cut into tiles of KMU_MINIMIZER_TILE consecutive windows; a read with nwin windows has
// ceil(nwin / TILE) tiles, a read without k-mers none.
//  k_mini_tiles       (kmu_seed_tiles.h) one lane per read: its number of tiles (u32).  A read shorter than k has no tile and no
//                     k-mer that would look at its bases: its bytes are validated there.  device_scan_u32 makes the tile offsets
//                     tile_off[n_seq + 1].
//  k_read_minimizers  one wave (a 64-thread workgroup) per tile, tiles dealt grid-stride; tile -> read by wave_find_read over
//                     tile_off.  The tile with windows [j0, j1) hashes the positions [j0 - 1, j1 - 1 + w) (clipped to the read)
//                     into LDS with SeqView + wave_step_kmers + apply_fhash: TILE + w - 1 positions for its own windows and one
//                     more in front, so that the window just before the tile is recomputed with the tile's own -- its choice
//                     says whether the choice of the tile's first window is new, and a minimizer whose windows lie on both
//                     sides of a tile boundary comes out once, from the tile that holds its first window.
//                     Sliding leftmost arg-min: every lane keeps (hash, position) of its entries e = c * 64 + lane in registers;
//                     a doubling pass d = 1, 2, 4, ... publishes them in LDS and takes min(own, entry e + d), the LEFT operand
//                     winning ties, so that after log2(D) passes (D the largest power of two <= w) an entry is the leftmost
//                     minimum of [e, e + D); the window's is min(entry e, entry e + w - D), left winning again.  Entries past the
//                     tile's positions read as u64::MAX and lie to the right of every real entry: they never win a tie.
//                     A window's choice is new iff it differs from the choice of the window in front (the first window of a
//                     read is always new); new choices are ranked by ballots in position order.
//                     COUNT leaves the number of new choices per tile, device_scan_u32 turns the counts into offsets, WRITE
//                     recomputes the tile and stores hash / position / read / strand at consecutive entries.  Recomputing costs
//                     a second pass over the bases (one byte per base); a bitmask of chosen positions from the first pass would
//                     need a workspace sized by the number of bases, which a KMU_MEM_DEVICE call does not know on the host.
//  k_mini_offsets     (kmu_seed_tiles.h) mini_offsets[i] = the offset of read i's first tile.
//  LDS: 10 KiB hashes + 2.5 KiB relative positions + 1.25 KiB strand bits = 13.75 KiB per one-wave workgroup (eleven per CU).
#include <algorithm>

#include "kmu_ctx.hpp"
#include "kmu_flat.h"
#include "kmu_seed_tiles.h"
#include "kmu_stream.h"

namespace kmu {

static constexpr uint32_t MINI_NE = KMU_MINIMIZER_TILE + KMU_MINIMIZER_MAX_W; // positions a tile holds at most: TILE + w
static constexpr uint32_t MINI_CH = MINI_NE / 64;                             // ... per lane
static_assert(MINI_NE % 64 == 0 && MINI_NE <= 65536, "a tile's entries are dealt to 64 lanes and indexed by 16 bits");

struct MiniArgs {
    const uint8_t *bases;
    const uint64_t *offsets;  // n_seq + 1
    const uint64_t *tile_off; // n_seq + 1: first tile of every read
    uint32_t n_seq;
    uint32_t w;
    uint64_t total_bytes;     // size of `bases`, or 0: offsets[n_seq]
    uint64_t room;            // COUNT: entries of `counts` (those behind the last tile are zeroed); WRITE: the number of tiles
    KmerCfg cfg;
    uint32_t *counts;         // COUNT: new choices per tile
    const uint64_t *coff;     // WRITE: first entry of every tile
    uint64_t *hashes;
    uint32_t *pos, *read;     // may be null
    uint8_t *strand;          // may be null
    uint32_t *err;
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_read_minimizers(MiniArgs a) {
    __shared__ uint64_t keys[MINI_NE];
    __shared__ uint16_t rpos[MINI_NE];
    __shared__ uint8_t strand[MINI_NE];
    const uint32_t lane = (uint32_t) lane_id();
    const int k = a.cfg.k;
    const uint32_t w = a.w;
    const uint64_t total = a.total_bytes ? a.total_bytes : a.offsets[a.n_seq];
    const uint64_t n_tiles = a.tile_off[a.n_seq];
    const bool canon = a.cfg.fhash == KMU_FHASH_CANON_RAW || a.cfg.fhash == KMU_FHASH_CANON_VALUE || a.cfg.fhash == KMU_FHASH_CANON_INVHASH;
    uint32_t D = 1; // the largest power of two <= w
    while (D * 2 <= w) D *= 2;
    const uint32_t tail = w - D;
    uint32_t bad = 0;
    for (uint64_t t = blockIdx.x; t < a.room; t += gridDim.x) {
        if (t >= n_tiles) { // (COUNT only: the counts array may be longer than the tiles)
            if (!WRITE && lane == 0) a.counts[t] = 0u;
            continue;
        }
        const uint32_t r = wave_find_read(a.tile_off, a.n_seq, t);
        const uint64_t rbeg = a.offsets[r], L = a.offsets[r + 1] - rbeg;
        const uint64_t nk = L - (uint64_t) k + 1; // > 0: the read has a tile
        const uint64_t nwin = nk > w ? nk - w + 1 : 1;
        const uint64_t j0 = (t - a.tile_off[r]) * MINI_T, j1 = std::min<uint64_t>(j0 + MINI_T, nwin);
        const uint64_t base = j0 ? j0 - 1 : 0;                         // first position held: the window in front of the tile starts here
        const uint64_t pend = std::min<uint64_t>(j1 - 1 + w, nk);      // one past the last
        const uint32_t n_real = (uint32_t) (pend - base);              // <= TILE + w
        const uint32_t nch = (n_real + 63) / 64;
        SeqView s;
        s.base = a.bases; s.begin = rbeg; s.len = L; s.total = total; s.packed = 0;
        const uint64_t lead = seq_lead(s);
        for (uint64_t st = (base + lead) / 1024; st <= (pend - 1 + lead) / 1024; st++)
            bad |= wave_step_kmers(s, k, st, base, pend, [&](uint64_t p, uint64_t val, uint64_t rc) {
                const uint32_t i = (uint32_t) (p - base);
                keys[i] = apply_fhash(a.cfg, val, rc);
                if (WRITE) strand[i] = (uint8_t) (canon && rc < val);
            });
        __syncthreads();
        uint64_t h[MINI_CH];
        uint32_t q[MINI_CH];
#pragma unroll
        for (uint32_t c = 0; c < MINI_CH; c++) {
            const uint32_t e = c * 64 + lane;
            h[c] = c < nch && e < n_real ? keys[e] : 0xFFFFFFFFFFFFFFFFull;
            q[c] = e;
        }
        // min(own, entry e + d) with the left operand winning ties; the state of the entries goes through LDS
        auto combine = [&](uint32_t d) {
#pragma unroll
            for (uint32_t c = 0; c < MINI_CH; c++)
                if (c < nch) {
                    const uint32_t e = c * 64 + lane;
                    keys[e] = h[c];
                    rpos[e] = (uint16_t) q[c];
                }
            __syncthreads();
#pragma unroll
            for (uint32_t c = 0; c < MINI_CH; c++)
                if (c < nch) {
                    const uint32_t e2 = c * 64 + lane + d;
                    if (e2 < n_real) {
                        const uint64_t nh = keys[e2];
                        const uint32_t nq = rpos[e2];
                        if (nh < h[c]) { h[c] = nh; q[c] = nq; }
                    }
                }
            __syncthreads();
        };
        for (uint32_t d = 1; d < D; d <<= 1) combine(d);
        if (tail) combine(tail);
        // the choice of the window in front of every window
#pragma unroll
        for (uint32_t c = 0; c < MINI_CH; c++)
            if (c < nch) rpos[c * 64 + lane] = (uint16_t) q[c];
        __syncthreads();
        const uint32_t wlo = (uint32_t) (j0 - base), whi = (uint32_t) (j1 - base); // the tile's own windows as entries
        const uint32_t nwc = (whi + 63) / 64;
        uint32_t run = 0;
        const uint64_t at = WRITE ? a.coff[t] : 0ull;
#pragma unroll
        for (uint32_t c = 0; c < MINI_CH; c++)
            if (c < nwc) {
                const uint32_t e = c * 64 + lane;
                // entry 0 is a window of the tile only when it is the first window of the read: always new
                const bool isnew = e >= wlo && e < whi && (e == 0 || rpos[e - 1] != (uint16_t) q[c]);
                const uint64_t bal = __ballot(isnew);
                if (WRITE && isnew) {
                    const uint64_t idx = at + run + (uint32_t) __popcll(bal & ((1ull << lane) - 1ull));
                    a.hashes[idx] = h[c];
                    if (a.pos) a.pos[idx] = (uint32_t) (base + q[c]);
                    if (a.read) a.read[idx] = r;
                    if (a.strand) a.strand[idx] = strand[q[c]];
                }
                run += (uint32_t) __popcll(bal);
            }
        if (!WRITE && lane == 0) a.counts[t] = run;
        __syncthreads(); // the next tile overwrites the LDS arrays
    }
    if (bad) atomicOr(a.err, DERR_NON_ACGT);
}

} // namespace kmu

using namespace kmu;

static bool mini_fhash_is_nthash(int fhash) { return fhash == KMU_FHASH_CANON_NTHASH || fhash == KMU_FHASH_CANON_NTHASH_8B; }

extern "C" int kmu_minimizer_layout(const uint64_t *offsets, uint32_t n_seq, uint32_t kmer_size, uint32_t w, uint64_t *out) {
    if (!offsets || !out || kmer_size == 0 || w == 0 || w > KMU_MINIMIZER_MAX_W) return KMU_E_BAD_ARG;
    out[0] = 0;
    for (uint32_t i = 0; i < n_seq; i++) out[i + 1] = out[i] + mini_windows(offsets[i + 1] - offsets[i], kmer_size, w);
    return KMU_OK;
}

extern "C" int kmu_read_minimizers(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                   uint32_t w, uint64_t *hashes_out, uint32_t *pos_out, uint32_t *read_out, uint8_t *strand_out,
                                   uint64_t cap, uint64_t *mini_offsets_out, uint64_t *n_out) {
    if (!ctx || !p || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null ctx, params or n_out");
    *n_out = 0;
    if (w == 0) return fail(ctx, KMU_E_BAD_ARG, "minimizers need a window of w >= 1 k-mers");
    if (w > KMU_MINIMIZER_MAX_W) return fail(ctx, KMU_E_UNSUPPORTED, "w = %u above KMU_MINIMIZER_MAX_W (%d)", w, KMU_MINIMIZER_MAX_W);
    const int mem = p->mem;
    KMU_TRY(check_mem(ctx, mem));
    if (kmer_is_aa(p->kmer_type)) return fail(ctx, KMU_E_BAD_ALPHABET, "minimizers are defined on DNA k-mers");
    if (p->input_kind == KMU_INPUT_PACKED2) return fail(ctx, KMU_E_UNSUPPORTED, "minimizers take unpacked (ASCII) bases");
    KMU_TRY(check_hash_params(ctx, p));
    if (strand_out && mini_fhash_is_nthash(p->fhash))
        return fail(ctx, KMU_E_UNSUPPORTED, "the canonical ntHash does not expose its strand: pass strand_out = NULL");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_seq == 0) {
        KMU_TRY(zero_first_offset(ctx, mini_offsets_out, mem));
        return finish_call(ctx, mem);
    }
    if (!offsets || !bases) return fail(ctx, KMU_E_BAD_ARG, "null sequence buffers");
    const uint32_t k = (uint32_t) p->kmer_size;
    // the number of tiles sizes the per-tile workspace.  Host arrays: counted here, with the length check.  Device arrays: the
    // workspace as large as it already is; the count below is done again if the tiles did not fit.
    uint64_t room = 0;
    if (mem == KMU_MEM_HOST) {
        for (uint32_t i = 0; i < n_seq; i++) {
            const uint64_t L = offsets[i + 1] - offsets[i];
            if (L > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "read %u has %llu bases: positions are uint32", i, (unsigned long long) L);
            room += (mini_windows(L, k, w) + MINI_T - 1) / MINI_T;
        }
        room = std::max<uint64_t>(room, 1);
    } else {
        room = std::max<uint64_t>(ctx->bufs["mini.counts"].bytes / 4, 1u << 16);
    }
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, mem, &ds));
    MiniArgs a{};
    a.bases = ds.bases;
    a.offsets = ds.offsets;
    a.n_seq = n_seq;
    a.w = w;
    a.total_bytes = ds.total_bytes;
    a.cfg = KmerCfg{p->kmer_type, p->kmer_size, p->fhash};
    KMU_TRY(get_err_word(ctx, &a.err));
    uint32_t *ntiles;
    uint64_t *tile_off;
    KMU_TRY(dev_array(ctx, "mini.ntiles", (size_t) n_seq + 1, &ntiles));
    KMU_TRY(dev_array(ctx, "mini.tile_off", (size_t) n_seq + 1, &tile_off));
    KMU_TRY(launch(ctx, nullptr, k_mini_tiles, dim3(grid_for(ctx, n_seq, 256)), dim3(256), 0, ds.bases, ds.offsets, n_seq, k, w, ntiles, a.err));
    KMU_TRY(device_scan_u32(ctx, ntiles, n_seq, tile_off));
    a.tile_off = tile_off;

    // COUNT, offsets, total
    uint64_t *coff = nullptr;
    uint64_t head[2] = {0, 0}; // tiles, minimizers
    for (;;) {
        if (room > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu tiles of windows: 2^32 or more", (unsigned long long) room);
        KMU_TRY(dev_array(ctx, "mini.counts", (size_t) room, &a.counts));
        KMU_TRY(dev_array(ctx, "mini.coff", (size_t) room + 1, &coff));
        a.room = room;
        const uint32_t grid = (uint32_t) std::min<uint64_t>(room, (uint64_t) ctx->num_cus * 40);
        KMU_TRY(launch(ctx, "k_read_minimizers_count", k_read_minimizers<false>, dim3(grid), dim3(64), 0, a));
        KMU_TRY(device_scan_u32(ctx, a.counts, room, coff));
        KMU_TRY(read_back(ctx, {{&head[0], tile_off + n_seq}, {&head[1], coff + room}}));
        if (head[0] <= room) break;
        room = head[0]; // (device arrays, more tiles than the workspace had room for)
    }
    const uint64_t n_tiles = head[0], total = head[1];
    *n_out = total;
    uint64_t *d_moff;
    KMU_TRY(place_output(ctx, "mini.moff", mini_offsets_out, (size_t) n_seq + 1, mem, &d_moff));
    if (mini_offsets_out) {
        KMU_TRY(launch(ctx, nullptr, k_mini_offsets, dim3(grid_for(ctx, (uint64_t) n_seq + 1, 256)), dim3(256), 0, tile_off, coff, n_seq, d_moff));
        KMU_TRY(bring_output(ctx, mini_offsets_out, d_moff, (size_t) n_seq + 1, mem));
    }
    if (!hashes_out || total == 0) return finish_checked(ctx, mem, a.err);
    if (cap < total) {
        KMU_TRY(finish_checked(ctx, mem, a.err));
        return fail(ctx, KMU_E_BAD_ARG, "%llu minimizers, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.room = n_tiles;
    a.coff = coff;
    KMU_TRY(place_output(ctx, "mini.hashes", hashes_out, (size_t) total, mem, &a.hashes));
    KMU_TRY(place_output(ctx, "mini.pos", pos_out, (size_t) total, mem, &a.pos));
    KMU_TRY(place_output(ctx, "mini.read", read_out, (size_t) total, mem, &a.read));
    KMU_TRY(place_output(ctx, "mini.strand", strand_out, (size_t) total, mem, &a.strand));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(n_tiles, (uint64_t) ctx->num_cus * 40);
    KMU_TRY(launch(ctx, "k_read_minimizers_write", k_read_minimizers<true>, dim3(grid), dim3(64), 0, a));
    KMU_TRY(bring_output(ctx, hashes_out, a.hashes, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, pos_out, a.pos, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, read_out, a.read, (size_t) total, mem));
    KMU_TRY(bring_output(ctx, strand_out, a.strand, (size_t) total, mem));
    return finish_checked(ctx, mem, a.err);
}

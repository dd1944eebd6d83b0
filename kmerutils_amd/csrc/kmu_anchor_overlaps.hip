// kmu_anchor_overlaps.hip -- from matched window pairs (kmu_anchor_match) to read pairs: a diagonal vote per read pair, on the
// device (kmu_anchor_overlaps; the semantics are in include/kmu.h).  A window pair (row a, row b) becomes, per strand, one ENTRY:
// its read pair, its diagonal, its weight and slice_a.  The entries are sorted by (read_a, read_b, strand, diagonal); equal keys
// are a RUN (one diagonal of one read pair), the runs of a read pair follow each other by strand and diagonal, and the winner of
// a read pair is the first of its runs with the largest band sum -- which is the tie rule (strand 0 first, then the smallest d).
//
//  k_ovl_keys   COUNT and WRITE.  One wave per tile of SORT_TILE window pairs, one lane per pair: the reads of both rows by binary
//               search in the row offsets, the KMU_OVL_UPPER test, survivors compacted in lane order by ballot and prefix count
//               (COUNT leaves one count per tile, device_scan_u32 makes the offsets; without the flag every pair survives and
//               COUNT is not run).  Pair c keeps (read_a << 32 | read_b), slice_a, slice_b and its weight; its entries
//               o = c * strands + s get the sort key (s << 32) | (d + 2^31) and the value o.  The number of entries stays on the
//               device (OvlInfo::n): every later kernel and the sort read it there, sized by the host's upper bound.
//  sort         radix_sort_pairs_passes on the diagonal key (4 passes, 5 with two strands); k_ovl_gather puts the read pair of
//               every entry in its place; radix_sort_pairs_passes on that (the bytes that n_reads_q and n_reads_db can reach).  The
//               sort is stable: the order is (read_a, read_b, strand, diagonal).
//  k_ovl_heads  one lane per sorted entry: does the run change here, does the read pair change here.  device_scan_u32 over each
//               flag array numbers runs and read pairs; k_run_starts (kmu_runs.h, shared with kmu_seed_chains.hip; profiled here
//               as k_ovl_starts) writes the first entry of every run and the first run of every read pair.
//  k_ovl_runs   one wave per run, runs dealt grid-stride: the lanes walk the run 64 entries at a time (a run of one read pair
//               matched on thousands of windows is no lane's alone), a wave reduction leaves weight (64 bits), min and max
//               slice_a; the number of entries is the distance to the next run.
//  k_ovl_best   COUNT and WRITE, so that the count-only call and the writing call walk identically.  One wave per read pair, one
//               lane per run: the band sum over the next <= band runs of the same strand of the same read pair whose diagonal is
//               within band, the lane's best (first of the largest), a wave argmax with the smaller run number on a tie, the
//               min_score filter.  COUNT leaves a 0/1 per read pair, device_scan_u32 the offsets, WRITE the records: ordered by
//               (read_a, read_b) because the read pairs are.
// Everything is integer arithmetic on sorted data; sums, counts, minima and maxima do not depend on the order inside a run, so
// the output does not depend on the order of the input.
#include <algorithm>

#include "kmu_runs.h"
#include "kmu_sort.h"

namespace kmu {

struct OvlInfo {
    uint64_t n;   // entries after KMU_OVL_UPPER
    uint32_t bad; // a last row offset that the diagonal field cannot hold
    uint32_t pad;
};

struct OvlArgs {
    const uint32_t *pairs, *dist; // n_pairs x 2, n_pairs x 3 or null
    uint64_t n_pairs;
    const uint64_t *off_q, *off_db; // n_reads + 1 each
    uint32_t n_reads_q, n_reads_db;
    uint32_t strands, band, min_score, upper;
    uint64_t n_max; // n_pairs * strands: the size every per-entry array has
    OvlInfo *info;
    // per surviving pair c
    uint64_t *prim;
    uint32_t *sa, *sb, *w;
    // per entry, sorted
    const uint64_t *skeys; // read pairs
    const uint32_t *svals; // entry numbers o = c * strands + s
    uint32_t *rhead, *phead, *keep;
    const uint64_t *ridx, *pidx; // exclusive scans of the flags; [n_max] = runs, read pairs
    uint32_t *rstart, *pstart;   // first entry of run r (and n behind the last); first run of read pair q (and runs behind the last)
    // per run
    uint64_t *rsec, *rw;
    uint32_t *rmin, *rmax;
    // output
    const uint64_t *ooff; // exclusive scan of keep; [n_max] = records
    uint64_t total;
    kmu_overlap *out;
};

// the read i with off[i] <= row < off[i + 1]; n >= 1.  A row behind the last offset is undefined input: it lands in the last read.
__device__ __forceinline__ uint32_t ovl_find_read(const uint64_t *off, uint32_t n, uint64_t row) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) { // first i with off[i + 1] > row
        const uint32_t mid = lo + (hi - lo) / 2;
        if (off[mid + 1] <= row) lo = mid + 1;
        else hi = mid;
    }
    return min(lo, n - 1);
}

// the diagonal key of entry o: (strand << 32) | (d + 2^31), d = slice_a - slice_b or slice_a + slice_b
__device__ __forceinline__ uint64_t ovl_sec(const OvlArgs &a, uint32_t o) {
    const uint32_t s = o & (a.strands - 1u), c = o >> (a.strands - 1u);
    const uint32_t sa = a.sa[c], sb = a.sb[c];
    return ((uint64_t) s << 32) | (uint32_t) ((s ? sa + sb : sa - sb) + 0x80000000u);
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_ovl_keys(OvlArgs a, uint32_t *counts, const uint64_t *coff,
                                                                        uint32_t n_tiles, uint64_t *keys, uint32_t *vals) {
    const uint32_t lane = (uint32_t) lane_id(), tile = blockIdx.x;
    const uint64_t below = (1ull << lane) - 1ull;
    const uint64_t t0 = (uint64_t) tile * SORT_TILE;
    uint64_t at = WRITE ? (coff ? coff[tile] : t0) : 0ull; // where the tile's next pair goes / how many it keeps so far
    if (WRITE && tile == 0 && lane == 0) {
        const uint64_t lq = a.off_q[a.n_reads_q], ldb = a.off_db[a.n_reads_db];
        a.info->n = (coff ? coff[n_tiles] : a.n_pairs) * a.strands;
        a.info->bad = (lq >= 0x80000000ull || ldb >= 0x80000000ull || (a.strands == 2 && lq + ldb > 0x80000000ull)) ? 1u : 0u;
        a.info->pad = 0;
    }
    for (uint32_t c0 = 0; c0 < SORT_TILE; c0 += 64) { // uniform trip count: all lanes reach the ballot
        const uint64_t p = t0 + c0 + lane;
        bool pass = p < a.n_pairs;
        uint32_t ra = 0, rb = 0, sa = 0, sb = 0;
        if (pass) {
            const uint32_t ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
            ra = ovl_find_read(a.off_q, a.n_reads_q, ia);
            rb = ovl_find_read(a.off_db, a.n_reads_db, ib);
            sa = ia - (uint32_t) a.off_q[ra];
            sb = ib - (uint32_t) a.off_db[rb];
            pass = !a.upper || ra < rb;
        }
        const uint64_t bal = __ballot(pass);
        if (WRITE) {
            const uint64_t c = at + (uint64_t) __popcll(bal & below);
            if (pass && c < a.n_pairs) {
                a.prim[c] = ((uint64_t) ra << 32) | rb;
                a.sa[c] = sa;
                a.sb[c] = sb;
                a.w[c] = a.dist ? a.dist[3 * p] : 1u;
                for (uint32_t s = 0; s < a.strands; s++) {
                    const uint64_t o = c * a.strands + s;
                    keys[o] = ((uint64_t) s << 32) | (uint32_t) ((s ? sa + sb : sa - sb) + 0x80000000u);
                    vals[o] = (uint32_t) o;
                }
            }
        }
        at += (uint64_t) __popcll(bal);
    }
    if (!WRITE && lane == 0) counts[tile] = (uint32_t) at;
}

// the read pair of every entry, in the order the first sort left
__global__ void __launch_bounds__(256) k_ovl_gather(OvlArgs a, const uint32_t *vals, uint64_t *keys) {
    const uint64_t n = min(a.info->n, a.n_max);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        keys[i] = a.prim[vals[i] >> (a.strands - 1u)];
}

// where a run begins and where a read pair begins; behind the last entry the flags are 0, and so is every keep
__global__ void __launch_bounds__(256) k_ovl_heads(OvlArgs a) {
    const uint64_t n = min(a.info->n, a.n_max);
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < a.n_max; i += (uint64_t) gridDim.x * blockDim.x) {
        uint32_t rh = 0, ph = 0;
        if (i < n) {
            ph = i == 0 || a.skeys[i] != a.skeys[i - 1];
            rh = ph || ovl_sec(a, a.svals[i]) != ovl_sec(a, a.svals[i - 1]);
        }
        a.rhead[i] = rh;
        a.phead[i] = ph;
        a.keep[i] = 0;
    }
}

__global__ void __launch_bounds__(64) k_ovl_runs(OvlArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_runs = a.ridx[a.n_max];
    for (uint64_t r = blockIdx.x; r < n_runs; r += gridDim.x) {
        const uint32_t beg = a.rstart[r], end = a.rstart[r + 1];
        uint64_t w = 0;
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (uint32_t i = beg + lane; i < end; i += 64) {
            const uint32_t c = a.svals[i] >> (a.strands - 1u);
            const uint32_t s = a.sa[c];
            w += a.w[c];
            mn = min(mn, s);
            mx = max(mx, s);
        }
        if (end - beg > 1) { // uniform
            w = wave_sum_u64(w);
            mn = wave_min_u32(mn);
            mx = wave_max_u32(mx);
        }
        if (lane == 0) {
            a.rsec[r] = ovl_sec(a, a.svals[beg]);
            a.rw[r] = w;
            a.rmin[r] = mn;
            a.rmax[r] = mx;
        }
    }
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_ovl_best(OvlArgs a) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_rp = a.pidx[a.n_max];
    for (uint64_t q = blockIdx.x; q < n_rp; q += gridDim.x) {
        if (WRITE && !a.keep[q]) continue; // uniform; COUNT decided it by the same walk
        const uint32_t beg = a.pstart[q], end = a.pstart[q + 1];
        uint64_t my_s = 0;
        uint32_t my_j = NONE, my_v = 0, my_mn = 0, my_mx = 0;
        for (uint32_t j = beg + lane; j < end; j += 64) {
            const uint64_t sec = a.rsec[j];
            uint64_t s = a.rw[j];
            uint32_t v = a.rstart[j + 1] - a.rstart[j], mn = a.rmin[j], mx = a.rmax[j];
            for (uint32_t t = 1; t <= a.band && j + t < end; t++) { // the band stops at the read pair, at the strand, at d + band
                const uint64_t sec2 = a.rsec[j + t];
                if ((sec2 >> 32) != (sec >> 32) || sec2 - sec > a.band) break;
                s += a.rw[j + t];
                v += a.rstart[j + t + 1] - a.rstart[j + t];
                mn = min(mn, a.rmin[j + t]);
                mx = max(mx, a.rmax[j + t]);
            }
            if (my_j == NONE || s > my_s) { // j ascends: the first of the largest stays
                my_s = s;
                my_j = j;
                my_v = v;
                my_mn = mn;
                my_mx = mx;
            }
        }
        uint64_t best_s = my_s;
        uint32_t best_j = my_j;
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) {
            const uint64_t os = ((uint64_t) (uint32_t) __shfl_xor((int) (best_s >> 32), d, 64) << 32) |
                                (uint32_t) __shfl_xor((int) (uint32_t) best_s, d, 64);
            const uint32_t oj = (uint32_t) __shfl_xor((int) best_j, d, 64);
            if (oj != NONE && (best_j == NONE || os > best_s || (os == best_s && oj < best_j))) {
                best_s = os;
                best_j = oj;
            }
        }
        const bool pass = best_j != NONE && best_s >= a.min_score;
        if (!WRITE) {
            if (lane == 0) a.keep[q] = pass ? 1u : 0u;
        } else if (pass && my_j == best_j) { // one lane: run numbers are distinct
            const uint64_t o = a.ooff[q];
            if (o < a.total) {
                const uint64_t rp = a.skeys[a.rstart[best_j]], sec = a.rsec[best_j];
                kmu_overlap rec;
                rec.read_a = (uint32_t) (rp >> 32);
                rec.read_b = (uint32_t) rp;
                rec.strand = (uint32_t) (sec >> 32);
                rec.diag = (int32_t) ((uint32_t) sec - 0x80000000u);
                rec.score = best_s > 0xFFFFFFFFull ? 0xFFFFFFFFu : (uint32_t) best_s;
                rec.votes = my_v;
                rec.slice_a_min = my_mn;
                rec.slice_a_max = my_mx;
                a.out[o] = rec;
            }
        }
    }
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_anchor_overlaps(kmu_ctx *ctx, const uint32_t *pairs, const uint32_t *dist, uint64_t n_pairs,
                                   const uint64_t *row_offsets_q, uint32_t n_reads_q, const uint64_t *row_offsets_db,
                                   uint32_t n_reads_db, uint32_t strands, uint32_t band, uint32_t min_score, uint32_t flags, int mem,
                                   kmu_overlap *out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !pairs || !row_offsets_q || !row_offsets_db || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (strands != 1 && strands != 2) return fail(ctx, KMU_E_BAD_ARG, "strands = %u: must be 1 or 2", strands);
    if (flags & ~KMU_OVL_UPPER) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", flags & ~KMU_OVL_UPPER);
    if (mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE) return fail(ctx, KMU_E_BAD_ARG, "bad mem %d", mem);
    if (band > KMU_OVL_MAX_BAND) return fail(ctx, KMU_E_UNSUPPORTED, "band = %u above KMU_OVL_MAX_BAND (%d)", band, KMU_OVL_MAX_BAND);
    if (n_pairs > 0xFFFFFFFFull / strands)
        return fail(ctx, KMU_E_UNSUPPORTED, "%llu pairs x %u strands: 2^32 entries or more", (unsigned long long) n_pairs, strands);
    const char *too_long = "a last row offset of 2^31 or more (or, with two strands, the two above 2^31 together): diagonals need 32 bits";
    if (mem == KMU_MEM_HOST) {
        const uint64_t lq = row_offsets_q[n_reads_q], ldb = row_offsets_db[n_reads_db];
        if (lq >= 0x80000000ull || ldb >= 0x80000000ull || (strands == 2 && lq + ldb > 0x80000000ull))
            return fail(ctx, KMU_E_UNSUPPORTED, "%s", too_long);
    }
    *n_out = 0;
    if (n_pairs == 0) return KMU_OK;
    if (n_reads_q == 0 || n_reads_db == 0) return fail(ctx, KMU_E_BAD_ARG, "pairs but no reads");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const uint64_t n_max = n_pairs * strands;
    const uint32_t n_tiles = (uint32_t) ((n_pairs + SORT_TILE - 1) / SORT_TILE);

    OvlArgs a{};
    const void *p;
    KMU_TRY(stage_to_device(ctx, "ovl.pairs", pairs, (size_t) n_pairs * 8, mem, &p));
    a.pairs = (const uint32_t *) p;
    KMU_TRY(stage_to_device(ctx, "ovl.dist", dist, (size_t) n_pairs * 12, mem, &p));
    a.dist = (const uint32_t *) p;
    KMU_TRY(stage_to_device(ctx, "ovl.offq", row_offsets_q, ((size_t) n_reads_q + 1) * 8, mem, &p));
    a.off_q = (const uint64_t *) p;
    if (row_offsets_db == row_offsets_q && n_reads_db == n_reads_q) a.off_db = a.off_q; // a self-join is staged once
    else {
        KMU_TRY(stage_to_device(ctx, "ovl.offdb", row_offsets_db, ((size_t) n_reads_db + 1) * 8, mem, &p));
        a.off_db = (const uint64_t *) p;
    }
    a.n_pairs = n_pairs;
    a.n_reads_q = n_reads_q;
    a.n_reads_db = n_reads_db;
    a.strands = strands;
    a.band = band;
    a.min_score = min_score;
    a.upper = (flags & KMU_OVL_UPPER) ? 1u : 0u;
    a.n_max = n_max;

    uint32_t *counts, *v0, *v1;
    uint64_t *coff, *k0, *k1, *ridx, *pidx, *ooff; // (the scans write what the kernels read through OvlArgs)
    KMU_TRY(dev_array(ctx, "ovl.info", 1, &a.info));
    KMU_TRY(dev_array(ctx, "ovl.counts", n_tiles, &counts));
    KMU_TRY(dev_array(ctx, "ovl.coff", (size_t) n_tiles + 1, &coff));
    KMU_TRY(dev_array(ctx, "ovl.prim", n_pairs, &a.prim));
    KMU_TRY(dev_array(ctx, "ovl.sa", n_pairs, &a.sa));
    KMU_TRY(dev_array(ctx, "ovl.sb", n_pairs, &a.sb));
    KMU_TRY(dev_array(ctx, "ovl.w", n_pairs, &a.w));
    KMU_TRY(dev_array(ctx, "ovl.keys0", n_max, &k0));
    KMU_TRY(dev_array(ctx, "ovl.vals0", n_max, &v0));
    KMU_TRY(dev_array(ctx, "ovl.keys1", n_max, &k1));
    KMU_TRY(dev_array(ctx, "ovl.vals1", n_max, &v1));
    KMU_TRY(dev_array(ctx, "ovl.rhead", n_max, &a.rhead));
    KMU_TRY(dev_array(ctx, "ovl.phead", n_max, &a.phead));
    KMU_TRY(dev_array(ctx, "ovl.keep", n_max, &a.keep));
    KMU_TRY(dev_array(ctx, "ovl.ridx", (size_t) n_max + 1, &ridx));
    KMU_TRY(dev_array(ctx, "ovl.pidx", (size_t) n_max + 1, &pidx));
    KMU_TRY(dev_array(ctx, "ovl.ooff", (size_t) n_max + 1, &ooff));
    KMU_TRY(dev_array(ctx, "ovl.rstart", (size_t) n_max + 1, &a.rstart));
    KMU_TRY(dev_array(ctx, "ovl.pstart", (size_t) n_max + 1, &a.pstart));
    KMU_TRY(dev_array(ctx, "ovl.rsec", n_max, &a.rsec));
    KMU_TRY(dev_array(ctx, "ovl.rw", n_max, &a.rw));
    KMU_TRY(dev_array(ctx, "ovl.rmin", n_max, &a.rmin));
    KMU_TRY(dev_array(ctx, "ovl.rmax", n_max, &a.rmax));
    a.ridx = ridx;
    a.pidx = pidx;
    a.ooff = ooff;
    const uint64_t *n_dev = &a.info->n;

    // entries
    if (a.upper) {
        KMU_TRY(launch(ctx, "k_ovl_keys_count", k_ovl_keys<false>, dim3(n_tiles), dim3(64), 0, a, counts, nullptr, n_tiles, k0, v0));
        KMU_TRY(device_scan_u32(ctx, counts, n_tiles, coff));
    }
    KMU_TRY(launch(ctx, "k_ovl_keys_write", k_ovl_keys<true>, dim3(n_tiles), dim3(64), 0, a, counts, a.upper ? coff : nullptr, n_tiles, k0, v0));

    // by diagonal, then (stable) by read pair
    const uint32_t flat = grid_for(ctx, n_max, 256);
    KMU_TRY(radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n_max, strands == 2 ? 0x1Fu : 0x0Fu, n_dev));
    KMU_TRY(launch(ctx, "k_ovl_gather", k_ovl_gather, dim3(flat), dim3(256), 0, a, v0, k0));
    KMU_TRY(radix_sort_pairs_passes(ctx, k0, v0, k1, v1, n_max, radix_id_passes(n_reads_db) | (radix_id_passes(n_reads_q) << 4), n_dev));
    a.skeys = k0;
    a.svals = v0;

    // runs and read pairs
    KMU_TRY(launch(ctx, "k_ovl_heads", k_ovl_heads, dim3(flat), dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.rhead, n_max, ridx));
    KMU_TRY(device_scan_u32(ctx, a.phead, n_max, pidx));
    KMU_TRY(launch(ctx, "k_ovl_starts", k_run_starts, dim3(flat), dim3(256), 0,
                   RunMarks{n_dev, n_max, a.rhead, a.phead, ridx, pidx, a.rstart, a.pstart}));
    const uint32_t waves = grid_for(ctx, n_max, 1, 32);
    KMU_TRY(launch(ctx, "k_ovl_runs", k_ovl_runs, dim3(waves), dim3(64), 0, a));

    // COUNT, offsets, total
    KMU_TRY(launch(ctx, "k_ovl_best_count", k_ovl_best<false>, dim3(waves), dim3(64), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.keep, n_max, ooff));
    uint64_t total = 0;
    OvlInfo h_info{};
    KMU_HIP(ctx, hipMemcpyAsync(&total, ooff + n_max, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipMemcpyAsync(&h_info, a.info, sizeof h_info, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (h_info.bad) { // (device memory: the offsets were read there)
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_UNSUPPORTED, "%s", too_long);
    }
    *n_out = total;
    if (!out || total == 0) return finish_call(ctx, mem);
    if (cap < total) {
        (void) finish_call(ctx, mem);
        return fail(ctx, KMU_E_BAD_ARG, "%llu overlaps, room for %llu", (unsigned long long) total, (unsigned long long) cap);
    }

    // WRITE
    a.total = total;
    a.out = out;
    if (mem == KMU_MEM_HOST) KMU_TRY(dev_array(ctx, "ovl.out", total, &a.out));
    KMU_TRY(launch(ctx, "k_ovl_best_write", k_ovl_best<true>, dim3(waves), dim3(64), 0, a));
    if (mem == KMU_MEM_HOST) KMU_HIP(ctx, hipMemcpyAsync(out, a.out, total * sizeof(kmu_overlap), hipMemcpyDeviceToHost, ctx->stream));
    return finish_call(ctx, mem);
}

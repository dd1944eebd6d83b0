// kmu_anchor_overlaps.hip -- from matched window pairs (kmu_anchor_match) to read pairs: a diagonal vote per read pair, on the
// device (kmu_anchor_overlaps; the semantics are in include/kmu.h).  A window pair (row a, row b) becomes, per strand, one ENTRY:
// its read pair, its diagonal, its weight and slice_a.  The entries are sorted by (read_a, read_b, strand, diagonal); equal keys
// are a RUN (one diagonal of one read pair), the runs of a read pair follow each other by strand and diagonal, and the winner of
// a read pair is the first of its runs with the largest band sum -- which is the tie rule (strand 0 first, then the smallest d).
//
//  k_ovl_keys   COUNT and WRITE: runs_compact of kmu_runs.h over OvlPairs, which says what a window pair is.  decode: the reads of
//               both rows by binary search in the row offsets, the KMU_OVL_UPPER test (pair 0 also looks at the last row offsets:
//               where the diagonal field cannot hold them it raises bad).  store: pair c keeps (read_a << 32 | read_b), slice_a,
//               slice_b and its weight; its entries o = c * strands + s get the sort key (s << 32) | (d + 2^31) and the value o.
//  grouping     runs_order of kmu_runs.h with that key as the inner key (4 sort passes, 5 with two strands): the order is
//               (read_a, read_b, strand, diagonal), a RUN is an inner unit.  Profiled as k_ovl_gather, k_ovl_heads, k_ovl_starts.
//  k_ovl_runs   one wave per run, runs dealt grid-stride: the lanes walk the run 64 entries at a time (a run of one read pair
//               matched on thousands of windows is no lane's alone), a wave reduction leaves weight (64 bits), min and max
//               slice_a; the number of entries is the distance to the next run.
//  k_ovl_best   COUNT and WRITE, so that the count-only call and the writing call walk identically.  One wave per read pair, one
//               lane per run: the band sum over the next <= band runs of the same strand of the same read pair whose diagonal is
//               within band, the lane's best (first of the largest), a wave argmax with the smaller run number on a tie, the
//               min_score filter.  COUNT leaves a 0/1 per read pair, runs_total the offsets and the total, WRITE the records:
//               ordered by (read_a, read_b) because the read pairs are.
// Everything is integer arithmetic on sorted data; sums, counts, minima and maxima do not depend on the order inside a run, so
// the output does not depend on the order of the input.
#include "kmu_runs.h"

namespace kmu {

struct OvlArgs {
    PairRuns r;                   // n_max = n_pairs * strands entries
    const uint32_t *pairs, *dist; // n_pairs x 2, n_pairs x 3 or null
    const uint64_t *off_q, *off_db; // n_reads + 1 each
    uint32_t n_reads_q, n_reads_db;
    uint32_t strands, band, min_score, upper;
    // per surviving pair c
    uint32_t *sa, *sb, *w;
    // per run
    uint64_t *rsec, *rw;
    uint32_t *rmin, *rmax;
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

// the diagonal key of strand s of a pair: (s << 32) | (d + 2^31), d = slice_a - slice_b or slice_a + slice_b
__device__ __forceinline__ uint64_t ovl_diag_key(uint32_t s, uint32_t sa, uint32_t sb) {
    return ((uint64_t) s << 32) | (uint32_t) ((s ? sa + sb : sa - sb) + 0x80000000u);
}
// the diagonal key of entry o
__device__ __forceinline__ uint64_t ovl_sec(const OvlArgs &a, uint32_t o) {
    const uint32_t s = o & (a.strands - 1u), c = o >> (a.strands - 1u);
    return ovl_diag_key(s, a.sa[c], a.sb[c]);
}

struct OvlPairs {
    struct Item {
        uint32_t ra, rb, sa, sb;
    };
    static __device__ __forceinline__ bool decode(const OvlArgs &a, uint64_t p, Item &it, uint32_t &bad) {
        if (p == 0) { // once per call (device memory: the host could not read the offsets)
            const uint64_t lq = a.off_q[a.n_reads_q], ldb = a.off_db[a.n_reads_db];
            if (lq >= 0x80000000ull || ldb >= 0x80000000ull || (a.strands == 2 && lq + ldb > 0x80000000ull)) bad = 1;
        }
        const uint32_t ia = a.pairs[2 * p], ib = a.pairs[2 * p + 1];
        it.ra = ovl_find_read(a.off_q, a.n_reads_q, ia);
        it.rb = ovl_find_read(a.off_db, a.n_reads_db, ib);
        it.sa = ia - (uint32_t) a.off_q[it.ra];
        it.sb = ib - (uint32_t) a.off_db[it.rb];
        return !a.upper || it.ra < it.rb;
    }
    static __device__ __forceinline__ void store(const OvlArgs &a, uint64_t p, uint64_t c, const Item &it) {
        a.r.prim[c] = ((uint64_t) it.ra << 32) | it.rb;
        a.sa[c] = it.sa;
        a.sb[c] = it.sb;
        a.w[c] = a.dist ? a.dist[3 * p] : 1u;
        for (uint32_t s = 0; s < a.strands; s++) {
            const uint64_t o = c * a.strands + s;
            a.r.skeys[o] = ovl_diag_key(s, it.sa, it.sb);
            a.r.svals[o] = (uint32_t) o;
        }
    }
    static __device__ __forceinline__ uint64_t inner(const OvlArgs &a, uint32_t v) { return ovl_sec(a, v); }
};

template <bool WRITE> __global__ void __launch_bounds__(64) k_ovl_keys(OvlArgs a) { runs_compact<OvlPairs, WRITE>(a); }

__global__ void __launch_bounds__(64) k_ovl_runs(OvlArgs a) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_runs = a.r.ridx[a.r.n_max];
    for (uint64_t r = blockIdx.x; r < n_runs; r += gridDim.x) {
        const uint32_t beg = a.r.rstart[r], end = a.r.rstart[r + 1];
        uint64_t w = 0;
        uint32_t mn = 0xFFFFFFFFu, mx = 0;
        for (uint32_t i = beg + lane; i < end; i += 64) {
            const uint32_t c = a.r.svals[i] >> (a.strands - 1u);
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
            a.rsec[r] = ovl_sec(a, a.r.svals[beg]);
            a.rw[r] = w;
            a.rmin[r] = mn;
            a.rmax[r] = mx;
        }
    }
}

template <bool WRITE> __global__ void __launch_bounds__(64) k_ovl_best(OvlArgs a) {
    constexpr uint32_t NONE = 0xFFFFFFFFu;
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t n_rp = a.r.pidx[a.r.n_max];
    for (uint64_t q = blockIdx.x; q < n_rp; q += gridDim.x) {
        if (WRITE && !a.r.keep[q]) continue; // uniform; COUNT decided it by the same walk
        const uint32_t beg = a.r.pstart[q], end = a.r.pstart[q + 1];
        uint64_t my_s = 0;
        uint32_t my_j = NONE, my_v = 0, my_mn = 0, my_mx = 0;
        for (uint32_t j = beg + lane; j < end; j += 64) {
            const uint64_t sec = a.rsec[j];
            uint64_t s = a.rw[j];
            uint32_t v = a.r.rstart[j + 1] - a.r.rstart[j], mn = a.rmin[j], mx = a.rmax[j];
            for (uint32_t t = 1; t <= a.band && j + t < end; t++) { // the band stops at the read pair, at the strand, at d + band
                const uint64_t sec2 = a.rsec[j + t];
                if ((sec2 >> 32) != (sec >> 32) || sec2 - sec > a.band) break;
                s += a.rw[j + t];
                v += a.r.rstart[j + t + 1] - a.r.rstart[j + t];
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
            if (lane == 0) a.r.keep[q] = pass ? 1u : 0u;
        } else if (pass && my_j == best_j) { // one lane: run numbers are distinct
            const uint64_t o = a.r.ooff[q];
            if (o < a.r.total) {
                const uint64_t rp = a.r.skeys[a.r.rstart[best_j]], sec = a.rsec[best_j];
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
    KMU_TRY(check_mem(ctx, mem));
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

    OvlArgs a{};
    KMU_TRY(stage_to_device(ctx, "ovl.pairs", pairs, (size_t) n_pairs * 2, mem, &a.pairs));
    KMU_TRY(stage_to_device(ctx, "ovl.dist", dist, (size_t) n_pairs * 3, mem, &a.dist));
    KMU_TRY(stage_to_device(ctx, "ovl.offq", row_offsets_q, (size_t) n_reads_q + 1, mem, &a.off_q));
    if (row_offsets_db == row_offsets_q && n_reads_db == n_reads_q) a.off_db = a.off_q; // a self-join is staged once
    else {
        KMU_TRY(stage_to_device(ctx, "ovl.offdb", row_offsets_db, (size_t) n_reads_db + 1, mem, &a.off_db));
    }
    a.n_reads_q = n_reads_q;
    a.n_reads_db = n_reads_db;
    a.strands = strands;
    a.band = band;
    a.min_score = min_score;
    a.upper = (flags & KMU_OVL_UPPER) ? 1u : 0u;

    KMU_TRY(runs_workspace(ctx, a.r, n_pairs, strands, strands - 1u, a.upper));
    const uint64_t n_max = a.r.n_max;
    KMU_TRY(dev_array(ctx, "ovl.sa", n_pairs, &a.sa));
    KMU_TRY(dev_array(ctx, "ovl.sb", n_pairs, &a.sb));
    KMU_TRY(dev_array(ctx, "ovl.w", n_pairs, &a.w));
    KMU_TRY(dev_array(ctx, "ovl.rsec", n_max, &a.rsec));
    KMU_TRY(dev_array(ctx, "ovl.rw", n_max, &a.rw));
    KMU_TRY(dev_array(ctx, "ovl.rmin", n_max, &a.rmin));
    KMU_TRY(dev_array(ctx, "ovl.rmax", n_max, &a.rmax));

    // entries; by diagonal, then (stable) by read pair; runs and read pairs
    KMU_TRY(runs_keys(ctx, "ovl", a, k_ovl_keys<false>, k_ovl_keys<true>));
    KMU_TRY(runs_order<OvlPairs>(ctx, "ovl", a, strands == 2 ? 0x1Fu : 0x0Fu, n_reads_q, n_reads_db));
    const uint32_t waves = grid_for(ctx, n_max, 1, 32);
    KMU_TRY(launch(ctx, "k_ovl_runs", k_ovl_runs, dim3(waves), dim3(64), 0, a));

    // COUNT, total, WRITE
    KMU_TRY(launch(ctx, "k_ovl_best_count", k_ovl_best<false>, dim3(waves), dim3(64), 0, a));
    bool emit;
    const int rc = runs_total(ctx, a.r, mem, out != nullptr, cap, n_out, "overlaps", too_long, &emit);
    if (!emit) return rc;
    return runs_emit(ctx, a.r, mem, out, [&](kmu_overlap *where) {
        a.out = where;
        return launch(ctx, "k_ovl_best_write", k_ovl_best<true>, dim3(waves), dim3(64), 0, a);
    });
}

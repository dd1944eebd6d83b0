// kmu_pile_segments.hip -- read trimming: the supported segments of every read with a class per read (kmu_pile_segments), and a new
// batch from byte ranges of a batch (kmu_extract_ranges).  The contracts are in include/kmu.h, the arithmetic in kmu_seg_core.h; the
// walk from the ranges' offsets to the output bytes is the segmented byte gather of kmu_gather.h.
//
// Tiles are SEG_TILE consecutive POSITIONS 0 .. n_rows of the batch, whatever read they belong to (position g stands for row g and for
// the end of row g - 1; kmu_seg_core.h says why), so a chromosome-long read is many waves' work.
//
//  k_seg_marks    one lane per read: sets the bit of its first row in a zeroed bitmap, one bit per position (atomic OR: empty reads
//                 set one bit several times).  The row pass learns the read boundaries from one 64-bit word per 64 rows.
//  k_seg_count    one wave per tile, one position per lane per trip: the row as one 16-byte and two 4-byte loads, (good, depth - ends)
//                 of the row before by a wave shift, and for lane 0 from the trip before (the tile's first trip loads that one row).
//                 Leaves the tile's number of starts and of ends.  device_scan_u32 turns both into tile offsets.
//  k_seg_write    the same walk: starts and ends are compacted separately by ballot and prefix count.  The k-th start and the k-th end
//                 are one run, because runs are disjoint and ordered; no run is ever followed across tiles.
//  k_seg_keep     one lane per run: its length, its read (a binary search over the offsets that takes the largest read, so empty reads
//                 are skipped), the length added to the read's n_good and, where the run is kept, 1 to the read's count (integer adds
//                 commute).  Two scans: where every kept run goes, and where every read's kept runs begin.
//  k_seg_place    one lane per run: a kept run becomes a record in read coordinates.
//  k_seg_reads    one lane per read over its kept segments: the ranks, the summary, and whether it has a segment at all.
//  k_seg_longest  (KMU_SEG_LONGEST) one lane per read that has one: its longest segment, at the scan of the "has" flags.
//  k_ext_lens     one lane per range: the check, and the length as two 32-bit halves (two scans make 64-bit offsets of them).
//  k_ext_offsets  one lane per range (and one for the end): out_offsets from the two scans (k_gather_offsets under this timer name).
//  k_ext_copy     gather_tiles over out_offsets: byte o of range r comes from begin[r] + (o - out_offsets[r]).
#include "kmu_ctx.hpp"
#include "kmu_gather.h"
#include "kmu_seg_core.h"

namespace kmu {

static_assert(sizeof(kmu_pile_seg) == 16 && sizeof(kmu_read_trim) == 32 && sizeof(kmu_pile_seg_params) == 16, "the records of the header");
static_assert(SEG_FLAG_LONGEST == KMU_SEG_LONGEST && SEG_WHOLE == KMU_TRIM_WHOLE && SEG_ENDS == KMU_TRIM_ENDS && SEG_SPLIT == KMU_TRIM_SPLIT &&
                  SEG_NONE == KMU_TRIM_NONE,
              "the flags and classes are the header's");

struct SegArgs {
    const uint32_t *pile;
    const uint64_t *off;       // [n_reads + 1]
    uint32_t n_reads;
    uint64_t n_rows, n_tiles;
    uint32_t min_depth, min_span, min_len;
    unsigned long long *marks; // [n_rows / 64 + 1]
    uint32_t *cnt_s, *cnt_e;   // [n_tiles]
    const uint64_t *soff, *eoff;
    uint64_t *starts, *ends;   // [n_runs]: rows of the batch; ends are exclusive
    uint64_t n_runs;
    uint32_t *keep, *run_read; // [n_runs]
    const uint64_t *koff;      // [n_runs + 1]: the kept runs before every run
    uint32_t *n_kept;          // [n_reads]
    const uint64_t *roff;      // [n_reads + 1]: the first kept segment of every read
    kmu_pile_seg *kept;        // every kept segment, in (read, start) order
    kmu_read_trim *reads;      // [n_reads]
    uint32_t *has;             // [n_reads]
    const uint64_t *loff;      // [n_reads + 1]
    kmu_pile_seg *longest;
};

__global__ void __launch_bounds__(256) k_seg_marks(SegArgs p) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < p.n_reads; r += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t g = p.off[r];
        if (g <= p.n_rows) atomicOr(p.marks + (g >> 6), 1ull << (g & 63u)); // (offsets that do not ascend to n_rows are the caller's fault)
    }
}

__device__ __forceinline__ SegRow seg_load_row(const SegArgs &p, uint64_t g) {
    uint32_t row[PILE_COLS] = {};
    const uint32_t *src = p.pile + g * PILE_COLS;
    const uint4 v = *reinterpret_cast<const uint4 *>(src);
    row[0] = v.x;
    row[1] = v.y;
    row[2] = v.z;
    row[3] = v.w;
    row[PILE_DEL] = src[PILE_DEL];
    row[PILE_ENDS] = src[PILE_ENDS];
    return seg_row(row, p.min_depth);
}

template <bool WRITE> __global__ void __launch_bounds__(256) k_seg_tiles(SegArgs p) {
    const uint32_t lane = (uint32_t) lane_id();
    const uint64_t below = lane ? ~0ull >> (64u - lane) : 0ull; // the lanes before this one
    for (uint64_t t = (uint64_t) blockIdx.x * 4u + (threadIdx.x >> 6); t < p.n_tiles; t += (uint64_t) gridDim.x * 4u) {
        const uint64_t base = t * SEG_TILE;
        SegRow carry = base > 0 && base - 1u < p.n_rows ? seg_load_row(p, base - 1u) : seg_no_row(); // (wave-uniform)
        uint32_t ns = 0, ne = 0;
        const uint64_t s0 = WRITE ? p.soff[t] : 0ull, e0 = WRITE ? p.eoff[t] : 0ull;
        for (uint32_t trip = 0; trip < SEG_TRIPS; trip++) {
            const uint64_t g0 = base + (uint64_t) trip * 64u, g = g0 + lane;
            if (g0 > p.n_rows) break; // (uniform: position n_rows is the last)
            const SegRow cur = g < p.n_rows ? seg_load_row(p, g) : seg_no_row();
            SegRow prev;
            prev.good = (uint32_t) __shfl_up((int) cur.good, 1, 64);
            prev.span = ((uint64_t) (uint32_t) __shfl_up((int) (cur.span >> 32), 1, 64) << 32) | (uint32_t) __shfl_up((int) (uint32_t) cur.span, 1, 64);
            if (lane == 0) prev = carry;
            carry.good = readlane_u32(cur.good, 63);
            carry.span = ((uint64_t) readlane_u32((uint32_t) (cur.span >> 32), 63) << 32) | readlane_u32((uint32_t) cur.span, 63);
            const bool marked = (p.marks[g0 >> 6] >> lane) & 1ull;
            const bool st = seg_is_start(prev, cur, marked, p.min_span), en = seg_is_end(prev, cur, st);
            const uint64_t bs = __ballot(st), be = __ballot(en);
            if (WRITE) {
                const uint64_t ks = s0 + ns + (uint32_t) __popcll(bs & below), ke = e0 + ne + (uint32_t) __popcll(be & below);
                if (st && ks < p.n_runs) p.starts[ks] = g;
                if (en && ke < p.n_runs) p.ends[ke] = g;
            }
            ns += (uint32_t) __popcll(bs);
            ne += (uint32_t) __popcll(be);
        }
        if (!WRITE && lane == 0) {
            p.cnt_s[t] = ns;
            p.cnt_e[t] = ne;
        }
    }
}

__global__ void __launch_bounds__(256) k_seg_keep(SegArgs p) {
    for (uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; k < p.n_runs; k += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t s = p.starts[k], e = p.ends[k];
        uint32_t keep = 0, r = 0;
        if (s < e && e <= p.n_rows) { // (always)
            r = (uint32_t) gather_upper_index(p.off, p.n_reads, s); // (at most n_reads)
            if (r < p.n_reads) {
                const uint32_t len = (uint32_t) (e - s);
                atomicAdd(&p.reads[r].n_good, len);
                keep = len >= p.min_len ? 1u : 0u;
                if (keep) atomicAdd(p.n_kept + r, 1u);
            }
        }
        p.keep[k] = keep;
        p.run_read[k] = r;
    }
}

__global__ void __launch_bounds__(256) k_seg_place(SegArgs p) {
    for (uint64_t k = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; k < p.n_runs; k += (uint64_t) gridDim.x * blockDim.x) {
        if (!p.keep[k]) continue;
        const uint32_t r = p.run_read[k];
        const uint64_t beg = p.off[r];
        kmu_pile_seg o;
        o.read = r;
        o.start = (uint32_t) (p.starts[k] - beg);
        o.end = (uint32_t) (p.ends[k] - beg);
        o.rank = 0;
        p.kept[p.koff[k]] = o; // (koff[k] < koff[n_runs] <= n_runs, the size of kept)
    }
}

__global__ void __launch_bounds__(256) k_seg_reads(SegArgs p) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < p.n_reads; r += (uint64_t) gridDim.x * blockDim.x) {
        SegSummary s = seg_summary_begin();
        for (uint64_t i = p.roff[r]; i < p.roff[r + 1]; i++) {
            seg_summary_add(s, p.kept[i].start, p.kept[i].end);
            p.kept[i].rank = (uint32_t) (i - p.roff[r]);
        }
        const uint64_t beg = p.off[r], end = p.off[r + 1];
        kmu_read_trim o;
        o.n_bases = end > beg ? (uint32_t) (end - beg) : 0u;
        o.n_good = p.reads[r].n_good; // (k_seg_keep has summed it)
        o.n_segs = s.n_segs;
        o.kept = s.kept;
        o.best_start = s.best_start;
        o.best_end = s.best_end;
        o.inner_bad = seg_inner_bad(s);
        o.cls = seg_class(s, o.n_bases);
        p.reads[r] = o;
        p.has[r] = s.n_segs ? 1u : 0u;
    }
}

__global__ void __launch_bounds__(256) k_seg_longest(SegArgs p) {
    for (uint64_t r = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; r < p.n_reads; r += (uint64_t) gridDim.x * blockDim.x) {
        if (!p.has[r]) continue;
        const kmu_read_trim t = p.reads[r];
        kmu_pile_seg o;
        o.read = (uint32_t) r;
        o.start = t.best_start;
        o.end = t.best_end;
        o.rank = 0;
        for (uint64_t i = p.roff[r]; i < p.roff[r + 1]; i++) // the first kept segment that is the best one: its rank
            if (p.kept[i].start == t.best_start) {
                o.rank = p.kept[i].rank;
                break;
            }
        p.longest[p.loff[r]] = o;
    }
}

// ---- kmu_extract_ranges ---------------------------------------------------------------------------------------------------------------
struct ExtArgs {
    const uint8_t *bases;
    uint64_t n_bases;
    const uint64_t *begin, *end;
    uint64_t n_ranges;
    uint32_t *len_lo, *len_hi, *info;
    const uint64_t *off_lo, *off_hi; // [n_ranges + 1]
    uint64_t *out_off;               // [n_ranges + 1]
    uint8_t *out;
    uint64_t total, n_tiles;
};

__global__ void __launch_bounds__(256) k_ext_lens(ExtArgs p) {
    bool bad = false;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < p.n_ranges; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint64_t b = p.begin[i], e = p.end[i];
        const bool ok = ext_range_ok(b, e, p.n_bases);
        const uint64_t len = ok ? e - b : 0ull;
        bad |= !ok;
        p.len_lo[i] = (uint32_t) len;
        p.len_hi[i] = (uint32_t) (len >> 32);
    }
    if (bad) p.info[0] = 1u;
}

__global__ void __launch_bounds__(256) k_ext_copy(ExtArgs p) {
    gather_tiles(p.out_off, p.n_ranges, p.total, p.n_tiles, [&](uint64_t r, uint64_t o) {
        const uint64_t src = p.begin[r] + (o - p.out_off[r]);
        if (r < p.n_ranges && src < p.n_bases) p.out[o] = p.bases[src]; // (k_ext_lens has checked the ranges: always)
    });
}

} // namespace kmu

using namespace kmu;

extern "C" int kmu_pile_segments(kmu_ctx *ctx, const uint32_t *pile, const uint64_t *offsets, uint32_t n_reads, const kmu_pile_seg_params *p, int mem,
                                 uint64_t *seg_offsets_out, kmu_pile_seg *segs_out, uint64_t cap, uint64_t *n_segs_out, kmu_read_trim *reads_out) {
    if (!ctx || !pile || !offsets || !p || !n_segs_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if (!seg_offsets_out && !reads_out && !segs_out) return fail(ctx, KMU_E_BAD_ARG, "no output");
    if (p->min_depth == 0) return fail(ctx, KMU_E_BAD_ARG, "min_depth must be at least 1");
    if (p->min_len == 0) return fail(ctx, KMU_E_BAD_ARG, "min_len must be at least 1");
    if (p->flags & ~KMU_SEG_LONGEST) return fail(ctx, KMU_E_BAD_ARG, "unknown flag bits 0x%x", p->flags);
    KMU_TRY(check_mem(ctx, mem));
    *n_segs_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_reads == 0) {
        KMU_TRY(zero_first_offset(ctx, seg_offsets_out, mem));
        if (seg_offsets_out) KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return KMU_OK;
    }
    uint64_t n_rows = 0;
    KMU_TRY(caller_word(ctx, offsets + n_reads, mem, &n_rows));
    const bool longest = p->flags & KMU_SEG_LONGEST;

    SegArgs a{};
    KMU_TRY(stage_to_device(ctx, "seg.pile", pile, (size_t) n_rows * PILE_COLS, mem, &a.pile));
    KMU_TRY(stage_to_device(ctx, "seg.off", offsets, (size_t) n_reads + 1, mem, &a.off));
    a.n_reads = n_reads;
    a.n_rows = n_rows;
    a.n_tiles = seg_n_tiles(n_rows);
    a.min_depth = p->min_depth;
    a.min_span = p->min_span;
    a.min_len = p->min_len;
    const size_t n_words = (size_t) (n_rows / 64u) + 1u;
    uint64_t *soff, *eoff, *roff, *loff;
    KMU_TRY(dev_array(ctx, "seg.marks", n_words, &a.marks));
    KMU_TRY(dev_array(ctx, "seg.cnts", a.n_tiles, &a.cnt_s));
    KMU_TRY(dev_array(ctx, "seg.cnte", a.n_tiles, &a.cnt_e));
    KMU_TRY(dev_array(ctx, "seg.soff", a.n_tiles + 1, &soff));
    KMU_TRY(dev_array(ctx, "seg.eoff", a.n_tiles + 1, &eoff));
    KMU_TRY(dev_array(ctx, "seg.nkept", n_reads, &a.n_kept));
    KMU_TRY(dev_array(ctx, "seg.roff", (size_t) n_reads + 1, &roff));
    KMU_TRY(dev_array(ctx, "seg.reads", n_reads, &a.reads));
    KMU_TRY(dev_array(ctx, "seg.has", n_reads, &a.has));
    KMU_TRY(dev_array(ctx, "seg.loff", (size_t) n_reads + 1, &loff));
    a.soff = soff;
    a.eoff = eoff;
    a.roff = roff;
    a.loff = loff;
    KMU_HIP(ctx, hipMemsetAsync(a.marks, 0, n_words * 8, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.n_kept, 0, (size_t) n_reads * 4, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(a.reads, 0, (size_t) n_reads * sizeof(kmu_read_trim), ctx->stream));

    // the row pass: marks, count, scans; the number of runs comes to the host (synchronisation)
    const dim3 grid_r(grid_for(ctx, n_reads, 256)), grid_t(grid_for(ctx, a.n_tiles, 4));
    KMU_TRY(launch(ctx, "k_seg_marks", k_seg_marks, grid_r, dim3(256), 0, a));
    KMU_TRY(launch(ctx, "k_seg_count", k_seg_tiles<false>, grid_t, dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.cnt_s, a.n_tiles, soff));
    KMU_TRY(device_scan_u32(ctx, a.cnt_e, a.n_tiles, eoff));
    uint64_t n_starts = 0, n_ends = 0;
    KMU_TRY(read_back(ctx, {{&n_starts, soff + a.n_tiles}, {&n_ends, eoff + a.n_tiles}}));
    if (n_starts != n_ends || n_starts > n_rows)
        return refuse(ctx, KMU_E_HIP, "internal: %llu starts and %llu ends", (unsigned long long) n_starts, (unsigned long long) n_ends);
    a.n_runs = n_starts;

    // the runs, what is kept of them, and where it goes
    uint64_t *koff;
    KMU_TRY(dev_array(ctx, "seg.starts", a.n_runs ? a.n_runs : 1, &a.starts));
    KMU_TRY(dev_array(ctx, "seg.ends", a.n_runs ? a.n_runs : 1, &a.ends));
    KMU_TRY(dev_array(ctx, "seg.keep", a.n_runs ? a.n_runs : 1, &a.keep));
    KMU_TRY(dev_array(ctx, "seg.runread", a.n_runs ? a.n_runs : 1, &a.run_read));
    KMU_TRY(dev_array(ctx, "seg.koff", a.n_runs + 1, &koff));
    KMU_TRY(dev_array(ctx, "seg.kept", a.n_runs ? a.n_runs : 1, &a.kept));
    a.koff = koff;
    if (a.n_runs) {
        const dim3 grid_k(grid_for(ctx, a.n_runs, 256));
        KMU_TRY(launch(ctx, "k_seg_write", k_seg_tiles<true>, grid_t, dim3(256), 0, a));
        KMU_TRY(launch(ctx, "k_seg_keep", k_seg_keep, grid_k, dim3(256), 0, a));
        KMU_TRY(device_scan_u32(ctx, a.keep, a.n_runs, koff));
        KMU_TRY(device_scan_u32(ctx, a.n_kept, n_reads, roff));
        KMU_TRY(launch(ctx, "k_seg_place", k_seg_place, grid_k, dim3(256), 0, a));
    } else {
        KMU_HIP(ctx, hipMemsetAsync(roff, 0, ((size_t) n_reads + 1) * 8, ctx->stream));
    }
    KMU_TRY(launch(ctx, "k_seg_reads", k_seg_reads, grid_r, dim3(256), 0, a));
    const uint64_t *out_off = roff;
    const kmu_pile_seg *out_segs = a.kept;
    if (longest) {
        KMU_TRY(dev_array(ctx, "seg.longest", n_reads, &a.longest));
        KMU_TRY(device_scan_u32(ctx, a.has, n_reads, loff));
        KMU_TRY(launch(ctx, "k_seg_longest", k_seg_longest, grid_r, dim3(256), 0, a));
        out_off = loff;
        out_segs = a.longest;
    }
    uint64_t total = 0;
    KMU_TRY(copy_out(ctx, seg_offsets_out, out_off, ((size_t) n_reads + 1) * 8, mem));
    KMU_TRY(copy_out(ctx, reads_out, a.reads, (size_t) n_reads * sizeof(kmu_read_trim), mem));
    KMU_TRY(read_back(ctx, {{&total, out_off + n_reads}}));
    *n_segs_out = total;
    if (segs_out && cap < total)
        return refuse(ctx, KMU_E_BAD_ARG, "cap = %llu is below the %llu segments", (unsigned long long) cap, (unsigned long long) total);
    if (segs_out && total) {
        KMU_TRY(copy_out(ctx, segs_out, out_segs, (size_t) total * sizeof(kmu_pile_seg), mem));
        return finish_sync(ctx);
    }
    return finish_synced(ctx);
}

extern "C" int kmu_extract_ranges(kmu_ctx *ctx, const uint8_t *bases, uint64_t n_bases, const uint64_t *begin, const uint64_t *end, uint64_t n_ranges,
                                  int mem, uint64_t *out_offsets, uint8_t *out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !out_offsets || !n_out) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    if ((!bases && n_bases) || ((!begin || !end) && n_ranges)) return fail(ctx, KMU_E_BAD_ARG, "null argument");
    KMU_TRY(check_mem(ctx, mem));
    *n_out = 0;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_ranges == 0) {
        KMU_TRY(zero_first_offset(ctx, out_offsets, mem));
        KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        return KMU_OK;
    }
    ExtArgs a{};
    KMU_TRY(stage_to_device(ctx, "ext.bases", bases, (size_t) n_bases, mem, &a.bases));
    a.n_bases = n_bases;
    KMU_TRY(stage_to_device(ctx, "ext.begin", begin, (size_t) n_ranges, mem, &a.begin));
    KMU_TRY(stage_to_device(ctx, "ext.end", end, (size_t) n_ranges, mem, &a.end));
    a.n_ranges = n_ranges;
    uint64_t *off_lo, *off_hi;
    KMU_TRY(dev_array(ctx, "ext.lenlo", n_ranges, &a.len_lo));
    KMU_TRY(dev_array(ctx, "ext.lenhi", n_ranges, &a.len_hi));
    KMU_TRY(dev_array(ctx, "ext.offlo", n_ranges + 1, &off_lo));
    KMU_TRY(dev_array(ctx, "ext.offhi", n_ranges + 1, &off_hi));
    KMU_TRY(dev_array(ctx, "ext.info", 1, &a.info));
    a.off_lo = off_lo;
    a.off_hi = off_hi;
    KMU_HIP(ctx, hipMemsetAsync(a.info, 0, 4, ctx->stream));

    // the check and the lengths; the refusal comes before any output (synchronisation)
    const dim3 grid_n(grid_for(ctx, n_ranges + 1, 256));
    KMU_TRY(launch(ctx, "k_ext_lens", k_ext_lens, grid_n, dim3(256), 0, a));
    KMU_TRY(device_scan_u32(ctx, a.len_lo, n_ranges, off_lo));
    KMU_TRY(device_scan_u32(ctx, a.len_hi, n_ranges, off_hi));
    uint32_t h_info = 0;
    uint64_t t_lo = 0, t_hi = 0;
    KMU_TRY(read_back(ctx, {{&h_info, a.info}, {&t_lo, off_lo + n_ranges}, {&t_hi, off_hi + n_ranges}}));
    if (h_info)
        return refuse(ctx, KMU_E_UNSUPPORTED, "a range with begin > end or end > n_bases = %llu", (unsigned long long) n_bases);
    a.total = t_lo + (t_hi << 32);
    a.n_tiles = (a.total + GATHER_TILE - 1u) / GATHER_TILE;
    KMU_TRY(place_output(ctx, "ext.outoff", out_offsets, n_ranges + 1, mem, &a.out_off));
    KMU_TRY(launch(ctx, "k_ext_offsets", k_gather_offsets, grid_n, dim3(256), 0, a.off_lo, a.off_hi, n_ranges, a.out_off));
    KMU_TRY(bring_output(ctx, out_offsets, a.out_off, n_ranges + 1, mem));
    *n_out = a.total;
    if (out && cap < a.total) {
        KMU_TRY(finish_sync(ctx));
        return fail(ctx, KMU_E_BAD_ARG, "cap = %llu is below the %llu bytes", (unsigned long long) cap, (unsigned long long) a.total);
    }
    if (out && a.total) {
        KMU_TRY(place_output(ctx, "ext.out", out, a.total, mem, &a.out));
        KMU_TRY(launch(ctx, "k_ext_copy", k_ext_copy, dim3(grid_for(ctx, a.n_tiles, 4)), dim3(256), 0, a));
        KMU_TRY(bring_output(ctx, out, a.out, a.total, mem));
    }
    return finish_sync(ctx);
}

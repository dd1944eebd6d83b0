// kmu_read_stats.hip -- the base and quality distributions of a batch (kmu_read_stats, kmu_read_qual_stats, kmu_quality_remap;
// include/kmu.h): get_base_count_par of the reference (src/statutils.rs:229-347) and its remap_quality8 (src/quality/quality.rs).
// The arithmetic is in kmu_rstat_core.h; DESIGN.md 3.27 has the argument.
//
// Both statistics are ONE kernel, a class histogram of a byte stream per read (k_rs_class_count over a classifier), and a second
// kernel with one thread per read that turns a read's counts into its record and feeds the batch's tables.
//   k_rs_class_count: a wave walks a region of 16 consecutive wave steps (16 KiB of the flat stream; 16 bytes per lane, 1 KiB per
//     step).  A step that lies inside one read is FAST: a lane counts its 16 bytes in byte-wide fields of one register, the fields
//     are widened to 16 bits and added to the lane's sums, which stay in registers while the read stays the same -- one wave
//     reduction and one set of atomic adds per (read, region), not per step.  A step in which reads end is SLOW: every lane walks
//     its bytes, moving on from read to read (runs of empty reads, many reads inside 16 bytes), and adds what it counted for a read
//     when it leaves it.
//   k_rs_reads / k_rq_reads: the record of a read; the 101 x 4 table through a histogram in LDS flushed once per workgroup, the
//     length histogram with one atomic per distinct bucket per wave, the totals through wave reductions.
// Every atomic is an integer add or max: the results do not depend on the schedule.
#include "kmu_ctx.hpp"
#include "kmu_flat.h"
#include "kmu_rstat_core.h"

namespace kmu {

static constexpr uint32_t RS_STEP = 1024, RS_REGION_STEPS = 16, RS_REGION = RS_STEP * RS_REGION_STEPS;

// the classifiers: NC classes; RAW: the sum, the minimum and the maximum of the raw bytes are kept too.  A read's row of
// accumulators is NC counts, then (RAW) the sum, 255 - the minimum and the maximum -- all start at 0 and only grow.
struct BaseClasses {
    static constexpr uint32_t NC = RS_BASE_CLASSES, ROW = NC;
    static constexpr bool RAW = false;
    static __device__ __forceinline__ uint32_t cls(uint32_t b) { return rs_base_class(b); }
};
struct QualClasses {
    static constexpr uint32_t NC = RS_QUAL_CLASSES, ROW = NC + 3;
    static constexpr bool RAW = true;
    static __device__ __forceinline__ uint32_t cls(uint32_t b) { return rs_qual_class(b); }
};

__device__ __forceinline__ void rs_add(unsigned long long *p, uint64_t v) {
    (void) __hip_atomic_fetch_add(p, (unsigned long long) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void rs_max(unsigned long long *p, uint64_t v) {
    (void) __hip_atomic_fetch_max(p, (unsigned long long) v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// what one lane counted for one read: the classes in byte-wide fields (at most 16 each), the raw bytes
struct LaneCount {
    uint64_t packed = 0;
    uint32_t sum = 0, mx = 0, mninv = 0;
};
template <class C> __device__ __forceinline__ void lane_count(LaneCount &c, uint32_t b) {
    c.packed += 1ull << (8u * C::cls(b));
    if (C::RAW) {
        c.sum += b;
        c.mx = b > c.mx ? b : c.mx;
        c.mninv = 255u - b > c.mninv ? 255u - b : c.mninv;
    }
}
// a lane's counts of read r into its row (the slow path)
template <class C> __device__ __forceinline__ void lane_flush(unsigned long long *acc, uint32_t r, LaneCount &c) {
    if (!c.packed) return;
    unsigned long long *row = acc + (uint64_t) r * C::ROW;
#pragma unroll
    for (uint32_t k = 0; k < C::NC; k++) {
        const uint32_t v = (uint32_t) (c.packed >> (8u * k)) & 0xFFu;
        if (v) rs_add(row + k, v);
    }
    if (C::RAW) {
        rs_add(row + C::NC, c.sum);
        rs_max(row + C::NC + 1, c.mninv);
        rs_max(row + C::NC + 2, c.mx);
    }
    c = LaneCount();
}

// acc[r * ROW + c] += the bytes of class c of read r, for the reads offsets[0 .. n_seq] of the stream; acc is zero on entry
template <class C>
__global__ void __launch_bounds__(256) k_rs_class_count(const uint8_t *bytes, const uint64_t *offsets, uint32_t n_seq, unsigned long long *acc) {
    const uint64_t start = offsets[0], total = offsets[n_seq];
    if (total <= start) return;
    const uint64_t rg_lo = start / RS_REGION, rg_hi = (total - 1) / RS_REGION + 1;
    const uint64_t wave_global = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    const uint32_t lane = (uint32_t) lane_id();
    uint32_t hint = 0xFFFFFFFFu;
    for (uint64_t rg = rg_lo + wave_global; rg < rg_hi; rg += nwaves) {
        // the wave's sums of read `cur` (wave-uniform), per lane in 16-bit fields: the even classes in lo, the odd ones in hi.  A
        // lane adds at most 16 per step and field: 256 in a region, 16 384 after the wave reduction.
        bool have = false;
        uint32_t cur = 0;
        uint64_t cur_end = 0, lo = 0, hi = 0;
        uint32_t sum = 0, mx = 0, mninv = 0;
        auto flush = [&]() {
            if (!have) return;
            lo = wave_sum_u64(lo);
            hi = wave_sum_u64(hi);
            unsigned long long *row = acc + (uint64_t) cur * C::ROW;
            if (lane < C::NC) {
                const uint32_t v = (uint32_t) (((lane & 1u) ? hi : lo) >> (16u * (lane >> 1))) & 0xFFFFu;
                if (v) rs_add(row + lane, v);
            }
            if (C::RAW) {
                sum = wave_sum_u32(sum); // (a lane: at most 16 * 16 * 255)
                mx = wave_max_u32(mx);
                mninv = wave_max_u32(mninv);
                if (lane == C::NC) rs_add(row + C::NC, sum);
                if (lane == C::NC + 1) rs_max(row + C::NC + 1, mninv);
                if (lane == C::NC + 2) rs_max(row + C::NC + 2, mx);
            }
            have = false;
            lo = hi = 0;
            sum = mx = mninv = 0;
        };
        for (uint32_t s = 0; s < RS_REGION_STEPS; s++) {
            const uint64_t s0 = rg * RS_REGION + (uint64_t) s * RS_STEP;
            if (s0 >= total) break;
            if (s0 + RS_STEP <= start) continue;
            const uint64_t a0 = s0 + 16u * lane;
            const uint4 v = load_chunk16(bytes, a0, total);
            const uint64_t x = ((uint64_t) v.y << 32) | v.x, y = ((uint64_t) v.w << 32) | v.z;
            if (!(have && s0 + RS_STEP <= cur_end)) {
                const uint32_t r = wave_find_read_from(offsets, n_seq, s0 > start ? s0 : start, hint); // the read of the step's first base
                hint = r;
                const uint64_t rend = offsets[r + 1];
                flush();
                if (s0 >= start && s0 + RS_STEP <= rend) { // the first whole step of another read
                    have = true;
                    cur = r;
                    cur_end = rend;
                } else { // reads end inside the step
                    const uint64_t g_lo = a0 > start ? a0 : start, g_hi = a0 + 16 < total ? a0 + 16 : total;
                    uint32_t rl = r;
                    uint64_t rl_end = rend;
                    LaneCount c;
#pragma unroll 1
                    for (uint32_t j = 0; j < 16; j++) {
                        const uint64_t g = a0 + j;
                        if (g < g_lo || g >= g_hi) continue;
                        if (g >= rl_end) {
                            lane_flush<C>(acc, rl, c);
                            while (g >= rl_end && rl + 1 < n_seq) { rl++; rl_end = offsets[rl + 1]; }
                        }
                        lane_count<C>(c, (uint32_t) ((j < 8 ? x >> (8u * j) : y >> (8u * (j - 8u))) & 0xFFu));
                    }
                    lane_flush<C>(acc, rl, c);
                    continue;
                }
            }
            LaneCount c;
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) lane_count<C>(c, (uint32_t) (x >> (8u * j)) & 0xFFu);
#pragma unroll
            for (uint32_t j = 0; j < 8; j++) lane_count<C>(c, (uint32_t) (y >> (8u * j)) & 0xFFu);
            lo += c.packed & 0x00FF00FF00FF00FFull;
            hi += (c.packed >> 8) & 0x00FF00FF00FF00FFull;
            if (C::RAW) {
                sum += c.sum;
                mx = c.mx > mx ? c.mx : mx;
                mninv = c.mninv > mninv ? c.mninv : mninv;
            }
        }
        flush();
    }
}

// scal: [0] bases, [1..4] A C G T, [5] other, [6] empty reads, [7] reads beyond the histogram, [8] max of ~length, [9] max length
enum : uint32_t { RSS_BASES = 0, RSS_BASE = 1, RSS_OTHER = 5, RSS_EMPTY = 6, RSS_OUT = 7, RSS_MIN_INV = 8, RSS_MAX = 9, RSS_WORDS = 16 };

__global__ void __launch_bounds__(256) k_rs_reads(const uint64_t *offsets, uint32_t n_seq, const unsigned long long *acc, uint32_t sub_bits,
                                                  uint64_t limit, kmu_read_comp *comp_out, unsigned long long *pct_hist,
                                                  unsigned long long *len_hist, unsigned long long *scal) {
    __shared__ uint32_t lh[RS_PCT_ROWS * 4];
    for (uint32_t t = threadIdx.x; t < RS_PCT_ROWS * 4; t += blockDim.x) lh[t] = 0;
    __syncthreads();
    const uint32_t lane = (uint32_t) lane_id();
    uint64_t t_base[4] = {0, 0, 0, 0}, t_bases = 0, t_other = 0, t_empty = 0, t_out = 0, t_mininv = 0, t_max = 0;
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t i0 = (uint64_t) blockIdx.x * blockDim.x + (threadIdx.x & ~63u); i0 < n_seq; i0 += stride) { // (wave-uniform trips)
        const uint64_t i = i0 + lane;
        const bool valid = i < n_seq;
        uint32_t bucket = RS_NO_BUCKET;
        if (valid) {
            const uint64_t len = offsets[i + 1] - offsets[i];
            const unsigned long long *row = acc + i * RS_BASE_CLASSES;
            kmu_read_comp c;
#pragma unroll
            for (uint32_t b = 0; b < 4; b++) {
                c.n_base[b] = row[b];
                c.pct[b] = (uint8_t) rs_pct(row[b], len);
                t_base[b] += row[b];
                if (pct_hist) atomicAdd(&lh[c.pct[b] * 4u + b], 1u);
            }
            c.n_other = row[4];
            if (len < limit) bucket = (uint32_t) rs_len_bucket(len, sub_bits);
            c.len_bucket = bucket;
            if (comp_out) comp_out[i] = c;
            t_bases += len;
            t_other += row[4];
            t_empty += len == 0;
            t_out += bucket == RS_NO_BUCKET;
            t_mininv = ~len > t_mininv ? ~len : t_mininv;
            t_max = len > t_max ? len : t_max;
        }
        // one add per distinct bucket of the wave
        bool pending = len_hist && bucket != RS_NO_BUCKET;
        for (;;) {
            const uint64_t m = __ballot(pending);
            if (!m) break;
            const uint32_t leader = (uint32_t) __ffsll((unsigned long long) m) - 1u;
            const uint32_t bb = bcast_u32(bucket, (int) leader);
            const bool same = pending && bucket == bb;
            const uint64_t ms = __ballot(same);
            if (lane == leader) rs_add(len_hist + bb, (uint64_t) __popcll(ms));
            if (same) pending = false;
        }
    }
    __syncthreads();
    if (pct_hist)
        for (uint32_t t = threadIdx.x; t < RS_PCT_ROWS * 4; t += blockDim.x)
            if (lh[t]) rs_add(pct_hist + t, lh[t]);
    t_bases = wave_sum_u64(t_bases);
    t_other = wave_sum_u64(t_other);
    t_empty = wave_sum_u64(t_empty);
    t_out = wave_sum_u64(t_out);
#pragma unroll
    for (uint32_t b = 0; b < 4; b++) t_base[b] = wave_sum_u64(t_base[b]);
    t_mininv = wave_max_u64(t_mininv);
    t_max = wave_max_u64(t_max);
    if (lane == 0) {
        if (t_bases) rs_add(scal + RSS_BASES, t_bases);
#pragma unroll
        for (uint32_t b = 0; b < 4; b++)
            if (t_base[b]) rs_add(scal + RSS_BASE + b, t_base[b]);
        if (t_other) rs_add(scal + RSS_OTHER, t_other);
        if (t_empty) rs_add(scal + RSS_EMPTY, t_empty);
        if (t_out) rs_add(scal + RSS_OUT, t_out);
        if (t_mininv) rs_max(scal + RSS_MIN_INV, t_mininv);
        if (t_max) rs_max(scal + RSS_MAX, t_max);
    }
}

__global__ void __launch_bounds__(256) k_rq_reads(const uint64_t *offsets, uint32_t n_seq, const unsigned long long *acc, kmu_read_qual *out,
                                                  unsigned long long *class_hist) {
    const uint32_t lane = (uint32_t) lane_id();
    uint64_t t_class[RS_QUAL_CLASSES] = {0, 0, 0, 0, 0, 0, 0, 0};
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += stride) {
        const uint64_t len = offsets[i + 1] - offsets[i];
        const unsigned long long *row = acc + i * QualClasses::ROW;
        kmu_read_qual q;
#pragma unroll
        for (uint32_t c = 0; c < RS_QUAL_CLASSES; c++) {
            q.n_class[c] = row[c];
            t_class[c] += row[c];
        }
        q.sum_q = row[RS_QUAL_CLASSES];
        q.min_q = (uint8_t) (255u - (uint32_t) row[RS_QUAL_CLASSES + 1]);
        q.max_q = (uint8_t) row[RS_QUAL_CLASSES + 2];
        q.median_class = (uint8_t) rs_median_class(q.n_class, len);
#pragma unroll
        for (uint32_t k = 0; k < 5; k++) q.pad[k] = 0;
        if (out) out[i] = q;
    }
    if (!class_hist) return; // (uniform)
#pragma unroll
    for (uint32_t c = 0; c < RS_QUAL_CLASSES; c++) {
        const uint64_t t = wave_sum_u64(t_class[c]);
        if (lane == c && t) rs_add(class_hist + c, t);
    }
}

// 16 bytes per thread where both arrays are 16-byte aligned, the bytes behind the last whole chunk (or all) one per thread
__global__ void __launch_bounds__(256) k_rq_remap(const uint8_t *quals, uint64_t n, uint64_t n_chunks, uint8_t *classes_out) {
    const uint64_t stride = (uint64_t) gridDim.x * blockDim.x, t0 = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x;
    for (uint64_t i = t0; i < n_chunks; i += stride) {
        const uint4 v = *reinterpret_cast<const uint4 *>(quals + 16 * i);
        uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (uint32_t k = 0; k < 4; k++) {
            uint32_t o = 0;
#pragma unroll
            for (uint32_t j = 0; j < 4; j++) o |= rs_qual_class((w[k] >> (8u * j)) & 0xFFu) << (8u * j);
            w[k] = o;
        }
        *reinterpret_cast<uint4 *>(classes_out + 16 * i) = make_uint4(w[0], w[1], w[2], w[3]);
    }
    for (uint64_t i = 16 * n_chunks + t0; i < n; i += stride) classes_out[i] = (uint8_t) rs_qual_class(quals[i]);
}

static bool rs_bad_mem(int mem) { return mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE; }

// the reads staged, their rows of accumulators zeroed and filled by k_rs_class_count
template <class C> static int rs_count(kmu_ctx *ctx, const char *kname, const uint8_t *bytes, const uint64_t *offsets, uint32_t n_seq, int mem,
                                       DevSeqs *ds, unsigned long long **acc_out) {
    KMU_TRY(stage_sequences(ctx, bytes, offsets, nullptr, n_seq, KMU_INPUT_ASCII, mem, ds));
    unsigned long long *acc;
    KMU_TRY(dev_array(ctx, "rs.acc", (size_t) n_seq * C::ROW + 1, &acc));
    KMU_HIP(ctx, hipMemsetAsync(acc, 0, ((size_t) n_seq * C::ROW + 1) * 8, ctx->stream));
    if (n_seq) KMU_TRY(launch(ctx, kname, k_rs_class_count<C>, dim3(ctx->num_cus * 8), dim3(256), 0, ds->bases, ds->offsets, n_seq, acc));
    *acc_out = acc;
    return KMU_OK;
}

} // namespace kmu

using namespace kmu;

extern "C" {

int kmu_len_hist_layout(uint64_t max_len, int sig_digits, uint32_t *n_buckets, uint64_t *limit) {
    const uint32_t sub_bits = rs_sub_bits(sig_digits);
    if (!sub_bits || !max_len || !n_buckets || !limit) return KMU_E_BAD_ARG;
    rs_len_layout(max_len, sub_bits, *n_buckets, *limit);
    return KMU_OK;
}

int kmu_len_bucket_range(int sig_digits, uint32_t bucket, uint64_t *lowest, uint64_t *highest) {
    const uint32_t sub_bits = rs_sub_bits(sig_digits);
    if (!sub_bits || !lowest || !highest) return KMU_E_BAD_ARG;
    rs_bucket_range(bucket, sub_bits, *lowest, *highest);
    return KMU_OK;
}

int kmu_read_stats(kmu_ctx *ctx, const kmu_read_stats_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                   kmu_read_comp *comp_out, uint64_t *pct_hist, uint64_t *len_hist, kmu_read_stats_info *info) {
    if (!ctx || !p || !info || !offsets || (!bases && n_seq) || rs_bad_mem(mem)) return fail(ctx, KMU_E_BAD_ARG, "kmu_read_stats: null argument or bad mem");
    const uint32_t sub_bits = rs_sub_bits(p->sig_digits);
    if (!sub_bits) return fail(ctx, KMU_E_BAD_ARG, "kmu_read_stats: sig_digits must be in [1, 5]");
    if (!p->max_len) return fail(ctx, KMU_E_BAD_ARG, "kmu_read_stats: max_len must be positive");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "kmu_read_stats_params.flags must be 0");
    uint32_t n_buckets;
    uint64_t limit;
    rs_len_layout(p->max_len, sub_bits, n_buckets, limit);
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    DevSeqs ds;
    unsigned long long *acc, *scal, *d_pct, *d_len;
    kmu_read_comp *d_comp;
    KMU_TRY(rs_count<BaseClasses>(ctx, "k_rs_base_count", bases, offsets, n_seq, mem, &ds, &acc));
    KMU_TRY(dev_array(ctx, "rs.scal", RSS_WORDS, &scal));
    KMU_TRY(place_output(ctx, "rs.comp", comp_out, (size_t) n_seq + 1, mem, &d_comp));
    KMU_TRY(place_output(ctx, "rs.pct", (unsigned long long *) pct_hist, RS_PCT_ROWS * 4 + 1, mem, &d_pct));
    KMU_TRY(place_output(ctx, "rs.len", (unsigned long long *) len_hist, (size_t) n_buckets + 1, mem, &d_len));
    KMU_HIP(ctx, hipMemsetAsync(scal, 0, RSS_WORDS * 8, ctx->stream));
    if (d_pct) KMU_HIP(ctx, hipMemsetAsync(d_pct, 0, RS_PCT_ROWS * 4 * 8, ctx->stream));
    if (d_len) KMU_HIP(ctx, hipMemsetAsync(d_len, 0, (size_t) n_buckets * 8, ctx->stream));
    if (n_seq)
        KMU_TRY(launch(ctx, "k_rs_reads", k_rs_reads, dim3(grid_for(ctx, n_seq, 256)), dim3(256), 0, ds.offsets, n_seq, acc, sub_bits, limit, d_comp,
                       d_pct, d_len, scal));
    if (mem == KMU_MEM_HOST) {
        KMU_TRY(copy_out(ctx, comp_out, d_comp, (size_t) n_seq * sizeof(kmu_read_comp), mem));
        KMU_TRY(copy_out(ctx, pct_hist, d_pct, RS_PCT_ROWS * 4 * 8, mem));
        KMU_TRY(copy_out(ctx, len_hist, d_len, (size_t) n_buckets * 8, mem));
    }
    uint64_t h[RSS_WORDS];
    KMU_HIP(ctx, hipMemcpyAsync(h, scal, sizeof h, hipMemcpyDeviceToHost, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the one synchronisation: info is the caller's, on the host)
    info->n_reads = n_seq;
    info->n_bases = h[RSS_BASES];
    for (int b = 0; b < 4; b++) info->n_base[b] = h[RSS_BASE + b];
    info->n_other = h[RSS_OTHER];
    info->n_empty = h[RSS_EMPTY];
    info->histo_out = h[RSS_OUT];
    info->min_len = n_seq ? ~h[RSS_MIN_INV] : 0;
    info->max_len = h[RSS_MAX];
    info->n_buckets = n_buckets;
    return finish_call(ctx, mem);
}

int kmu_quality_remap(kmu_ctx *ctx, const uint8_t *quals, uint64_t n, int mem, uint8_t *classes_out) {
    if (!ctx || ((!quals || !classes_out) && n) || rs_bad_mem(mem)) return fail(ctx, KMU_E_BAD_ARG, "kmu_quality_remap: null argument or bad mem");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return KMU_OK;
    const uint8_t *d_q;
    KMU_TRY(stage_to_device(ctx, "rq.in", quals, n, mem, &d_q));
    uint8_t *d_o;
    KMU_TRY(place_output(ctx, "rq.out", classes_out, n + 17, mem, &d_o));
    const uint64_t n_chunks = (((uintptr_t) d_q | (uintptr_t) d_o) & 15u) ? 0 : n / 16;
    KMU_TRY(launch(ctx, "k_rq_remap", k_rq_remap, dim3(grid_for(ctx, n_chunks + 256, 256)), dim3(256), 0, d_q, n, n_chunks, d_o));
    if (mem == KMU_MEM_HOST) KMU_TRY(copy_out(ctx, classes_out, d_o, n, mem));
    return finish_call(ctx, mem);
}

int kmu_read_qual_stats(kmu_ctx *ctx, const uint8_t *quals, const uint64_t *offsets, uint32_t n_seq, int mem, kmu_read_qual *out,
                        uint64_t *class_hist) {
    if (!ctx || !offsets || (!quals && n_seq) || rs_bad_mem(mem)) return fail(ctx, KMU_E_BAD_ARG, "kmu_read_qual_stats: null argument or bad mem");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    DevSeqs ds;
    unsigned long long *acc, *d_hist;
    kmu_read_qual *d_out;
    KMU_TRY(rs_count<QualClasses>(ctx, "k_rs_qual_count", quals, offsets, n_seq, mem, &ds, &acc));
    KMU_TRY(place_output(ctx, "rq.reads", out, (size_t) n_seq + 1, mem, &d_out));
    KMU_TRY(place_output(ctx, "rq.hist", (unsigned long long *) class_hist, RS_QUAL_CLASSES + 1, mem, &d_hist));
    if (d_hist) KMU_HIP(ctx, hipMemsetAsync(d_hist, 0, RS_QUAL_CLASSES * 8, ctx->stream));
    if (n_seq) KMU_TRY(launch(ctx, "k_rq_reads", k_rq_reads, dim3(grid_for(ctx, n_seq, 256)), dim3(256), 0, ds.offsets, n_seq, acc, d_out, d_hist));
    if (mem == KMU_MEM_HOST) {
        KMU_TRY(copy_out(ctx, out, d_out, (size_t) n_seq * sizeof(kmu_read_qual), mem));
        KMU_TRY(copy_out(ctx, class_hist, d_hist, RS_QUAL_CLASSES * 8, mem));
    }
    return finish_call(ctx, mem);
}

} // extern "C"

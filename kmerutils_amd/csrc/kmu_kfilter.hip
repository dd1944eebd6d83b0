// kmu_kfilter.hip -- the count prefilter (kmu_kfilter, include/kmu.h): a two-plane Bloom filter that tells the k-mers seen once
// from those seen more often, built in a first pass over the reads so that a second pass counts only the k-mers that may occur
// twice (kmu_count_add_reads_filtered).  The arithmetic of a key is in kmu_kfilter_core.h; DESIGN.md 3.26 has the argument.
//
// Adding one occurrence of v:  old = atomic_or(&A[cell], mask);  rep = old & mask;  if (rep) atomic_or(&B[cell], rep).
// Atomics on one word are totally ordered, so the final planes are a pure function of the MULTISET of occurrences: A[c] = OR of
// the masks that landed in c, bit b of B[c] = "at least two occurrences landed on bit b of c" -- whatever the order, the launch
// shape or the number of add calls.  Every atomic here is relaxed, agent scope: the planes are read by later kernels only.
#include <algorithm>
#include <vector>

#include "kmu_count_table.h"
#include "kmu_flat.h"
#include "kmu_kfilter_core.h"

struct kmu_kfilter {
    kmu_ctx *ctx = nullptr;
    kmu_kfilter_params p{};
    uint64_t *cells = nullptr;   // device: n_cells x {A, B}
    uint64_t *scalars = nullptr; // device: [0] occurrences added, [1] / [2] popcounts of the planes (kmu_kfilter_info)
};

namespace kmu {

struct KfView {
    uint64_t *cells;
    uint64_t n_cells;
    uint32_t n_hashes;
};

__device__ __forceinline__ uint64_t kf_or(uint64_t *p, uint64_t m) { return __hip_atomic_fetch_or(p, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// one 16-byte load of the cell of v: 0 / 1 / 2
__device__ __forceinline__ uint32_t kf_lookup(const KfView &f, uint64_t v) {
    uint64_t cell, mask;
    kf_cell_mask(v, f.n_cells, f.n_hashes, cell, mask);
    const uint4 c = *reinterpret_cast<const uint4 *>(f.cells + 2 * cell);
    return kf_class(((uint64_t) c.y << 32) | c.x, ((uint64_t) c.w << 32) | c.z, mask);
}

// The walk of k_count_add_flat.  A lane's k-mers of a step are independent: their returning ORs on plane A are all issued before
// any result is looked at (up to 16 in flight), then the no-return ORs on plane B.
__global__ void __launch_bounds__(256) k_kf_add_flat(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, KfView f,
                                                     uint64_t *n_added, uint32_t *err) {
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t nsteps = flat_wave_steps(total);
    const uint64_t wave_global = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves_global = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    uint32_t anybad = 0, r_hint = 0xFFFFFFFFu;
    uint64_t added = 0;
    for (uint64_t st = wave_global; st < nsteps; st += nwaves_global) {
        uint64_t *pa[16], mask[16], old[16];
        uint32_t valid = 0;
        anybad |= flat_step_visit<true>(bases, offsets, n_seq, total, start, k, st, r_hint, [&](int j, uint64_t canon, uint32_t) {
            uint64_t cell;
            kf_cell_mask(canon, f.n_cells, f.n_hashes, cell, mask[j]);
            pa[j] = f.cells + 2 * cell;
            valid |= 1u << j;
        });
        if (__all(valid == 0xFFFFu || valid == 0u)) { // (long reads: nearly every wave)
            if (valid) {
#pragma unroll
                for (int j = 0; j < 16; j++) old[j] = kf_or(pa[j], mask[j]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 16; j++) old[j] = (valid >> j) & 1u ? kf_or(pa[j], mask[j]) : 0ull;
        }
        // every result is looked at here, once (one wait for all of them): the ORs on B then wait for nothing
        uint64_t any = 0;
#pragma unroll
        for (int j = 0; j < 16; j++) {
            old[j] = (valid >> j) & 1u ? old[j] & mask[j] : 0ull;
            any |= old[j];
        }
        if (any) {
#pragma unroll
            for (int j = 0; j < 16; j++)
                if (old[j]) (void) kf_or(pa[j] + 1, old[j]);
        }
        added += (uint32_t) __popc(valid);
    }
    added = wave_sum_u64(added);
    if (lane_id() == 0 && added) atomicAdd((unsigned long long *) n_added, (unsigned long long) added);
    if (anybad) atomicOr(err, DERR_NON_ACGT);
}

__global__ void __launch_bounds__(256) k_kf_add_kmers(const uint64_t *kmers, uint64_t n, KfView f, uint64_t *n_added) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) {
        uint64_t cell, mask;
        kf_cell_mask(kmers[i], f.n_cells, f.n_hashes, cell, mask);
        const uint64_t rep = kf_or(f.cells + 2 * cell, mask) & mask;
        if (rep) (void) kf_or(f.cells + 2 * cell + 1, rep);
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) atomicAdd((unsigned long long *) n_added, (unsigned long long) n);
}

__global__ void __launch_bounds__(256) k_kf_query(const uint64_t *kmers, uint64_t n, KfView f, uint8_t *class_out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x)
        class_out[i] = (uint8_t) kf_lookup(f, kmers[i]);
}

// scalars[1] += set bits of plane A, [2] += of plane B
__global__ void __launch_bounds__(256) k_kf_popcount(const uint64_t *cells, uint64_t n_cells, uint64_t *scalars) {
    uint64_t a = 0, b = 0;
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t) gridDim.x * blockDim.x) {
        const uint4 c = *reinterpret_cast<const uint4 *>(cells + 2 * i);
        a += (uint32_t) (__popc(c.x) + __popc(c.y));
        b += (uint32_t) (__popc(c.z) + __popc(c.w));
    }
    a = wave_sum_u64(a);
    b = wave_sum_u64(b);
    if (lane_id() == 0) {
        if (a) atomicAdd((unsigned long long *) &scalars[1], (unsigned long long) a);
        if (b) atomicAdd((unsigned long long *) &scalars[2], (unsigned long long) b);
    }
}

// dst becomes the filter of the concatenated input: A = A1 | A2, B = B1 | B2 | (A1 & A2); the occurrences add up
__global__ void __launch_bounds__(256) k_kf_merge(uint64_t *dst, const uint64_t *src, uint64_t n_cells, uint64_t *dst_scalars,
                                                  const uint64_t *src_scalars) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n_cells; i += (uint64_t) gridDim.x * blockDim.x) {
        uint4 d = *reinterpret_cast<const uint4 *>(dst + 2 * i);
        const uint4 s = *reinterpret_cast<const uint4 *>(src + 2 * i);
        d.z |= s.z | (d.x & s.x);
        d.w |= s.w | (d.y & s.y);
        d.x |= s.x;
        d.y |= s.y;
        *reinterpret_cast<uint4 *>(dst + 2 * i) = d;
    }
    if (blockIdx.x == 0 && threadIdx.x == 0) dst_scalars[0] += src_scalars[0];
}

// ---- the occurrences the filter lets pass (class 2), in (sequence, position) order: the count / scan / write of k_once_count and
// k_once_emit (kmu_count.hip) with the class test in the place of the table look-up -----------------------------------------------
__device__ __forceinline__ uint32_t pass_step(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, uint64_t total, uint64_t start,
                                              int k, uint64_t st, uint32_t &r_hint, const KfView &f, uint64_t (&canon)[16], uint32_t &bad) {
    uint32_t mask = 0;
    bad |= flat_step_visit<false>(bases, offsets, n_seq, total, start, k, st, r_hint, [&](int j, uint64_t c, uint32_t) {
        if (kf_lookup(f, c) == 2u) {
            mask |= 1u << j;
            canon[j] = c;
        }
    });
    return mask;
}

__global__ void __launch_bounds__(256) k_kf_pass_count(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, KfView f,
                                                       uint32_t *cnt, uint32_t *err) {
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t nsteps = flat_wave_steps(total);
    const uint64_t wave_global = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves_global = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    uint32_t r_hint = 0xFFFFFFFFu, anybad = 0;
    for (uint64_t st = wave_global; st < nsteps; st += nwaves_global) {
        uint64_t canon[16];
        const uint32_t mask = pass_step(bases, offsets, n_seq, total, start, k, st, r_hint, f, canon, anybad);
        const uint32_t incl = wave_incl_scan_u32((uint32_t) __popc(mask));
        if (lane_id() == 63) cnt[st] = incl;
    }
    if (anybad) atomicOr(err, DERR_NON_ACGT);
}

// the same walk over the steps [st_lo, st_hi); step st writes its k-mers at base[st] - base[st_lo] ..
__global__ void __launch_bounds__(256) k_kf_pass_emit(const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int k, KfView f,
                                                      const uint64_t *base, uint64_t st_lo, uint64_t st_hi, uint64_t *kmers_out) {
    const uint64_t total = offsets[n_seq], start = offsets[0];
    const uint64_t wave_global = ((uint64_t) blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    const uint64_t nwaves_global = ((uint64_t) gridDim.x * blockDim.x) >> 6;
    const uint64_t base_lo = base[st_lo];
    uint32_t r_hint = 0xFFFFFFFFu, bad = 0;
    for (uint64_t st = st_lo + wave_global; st < st_hi; st += nwaves_global) {
        uint64_t canon[16];
        const uint32_t mask = pass_step(bases, offsets, n_seq, total, start, k, st, r_hint, f, canon, bad);
        const uint32_t c = (uint32_t) __popc(mask);
        uint64_t at = base[st] - base_lo + (wave_incl_scan_u32(c) - c);
#pragma unroll
        for (int j = 0; j < 16; j++)
            if ((mask >> j) & 1u) kmers_out[at++] = canon[j];
    }
}

// The wave steps cut into consecutive ranges whose survivors fit `cap` k-mers (cap >= 1024: one step always fits).  One thread:
// cut[2 i] = the first step of range i, cut[2 i + 1] = base[that step]; the entry after the last range closes it (nsteps, total);
// *n_ranges <= max_ranges.  Every range but the last holds more than cap - 1024 survivors, which bounds their number.
__global__ void k_kf_cut(const uint64_t *base, uint64_t nsteps, uint64_t cap, uint64_t max_ranges, uint64_t *cut, uint64_t *n_ranges) {
    if (blockIdx.x || threadIdx.x) return;
    uint64_t lo = 0, n = 0;
    cut[0] = 0;
    cut[1] = base[0];
    while (lo < nsteps && n < max_ranges) {
        uint64_t a = lo + 1, b = nsteps; // the largest a in (lo, nsteps] with base[a] - base[lo] <= cap
        while (a < b) {
            const uint64_t mid = a + (b - a + 1) / 2;
            if (base[mid] - base[lo] <= cap) a = mid;
            else b = mid - 1;
        }
        n++;
        cut[2 * n] = a;
        cut[2 * n + 1] = base[a];
        lo = a;
    }
    *n_ranges = n;
}

static KfView view_of(const kmu_kfilter *f) { return KfView{f->cells, f->p.n_cells, f->p.n_hashes}; }

// what both passes over the reads share: the reads staged, the extent of their flat stream
struct KfReads {
    DevSeqs ds;
    uint64_t total_bases = 0;
};
static int kf_stage(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem, KfReads *r) {
    kmu_ctx *ctx = f->ctx;
    KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, mem, &r->ds));
    if (n_seq) KMU_TRY(flat_stream_extent(ctx, offsets, n_seq, mem, r->ds, &r->total_bases));
    return KMU_OK;
}

// k_kf_pass_count and the scan: base[st] = the survivors before step st, base[nsteps] their number
static int kf_pass_scan(kmu_kfilter *f, const KfReads &r, uint32_t *d_err, uint64_t **base_out, uint64_t *nsteps_out, int *grid_out) {
    kmu_ctx *ctx = f->ctx;
    const uint64_t nsteps = flat_wave_steps(r.total_bases);
    uint64_t *base;
    uint32_t *cnt;
    KMU_TRY(dev_array(ctx, "kf.cnt", nsteps + 16, &cnt));
    KMU_TRY(dev_array(ctx, "kf.base", nsteps + 1 + 8, &base));
    const int grid = grid_for(ctx, nsteps, 4);
    KMU_TRY(launch(ctx, "k_kf_pass_count", k_kf_pass_count, dim3(grid), dim3(256), 0, r.ds.bases, r.ds.offsets, r.ds.n_seq, f->p.kmer_size,
                   view_of(f), cnt, d_err));
    KMU_TRY(device_scan_u32(ctx, cnt, nsteps, base));
    *base_out = base;
    *nsteps_out = nsteps;
    *grid_out = grid;
    return KMU_OK;
}

static bool kf_bad_mem(int mem) { return mem != KMU_MEM_HOST && mem != KMU_MEM_DEVICE; }

} // namespace kmu

using namespace kmu;

extern "C" {

uint64_t kmu_kfilter_cells_for(uint64_t expected_distinct, uint32_t bits_per_kmer) { return kf_cells_for(expected_distinct, bits_per_kmer); }

int kmu_kfilter_create(kmu_ctx *ctx, const kmu_kfilter_params *p, kmu_kfilter **out) {
    if (!ctx || !p || !out) return KMU_E_BAD_ARG;
    *out = nullptr;
    KMU_TRY(check_kmer(ctx, p->kmer_type, p->kmer_size));
    if (kmer_is_aa(p->kmer_type)) return fail(ctx, KMU_E_BAD_ARG, "the count prefilter is defined on DNA k-mers (canonical form)");
    if (p->n_hashes < 1 || p->n_hashes > KF_MAX_HASHES) return fail(ctx, KMU_E_BAD_ARG, "n_hashes must be in [1, 8]");
    if (p->n_cells < 1 || p->n_cells > KF_MAX_CELLS) return fail(ctx, KMU_E_BAD_ARG, "n_cells must be in [1, 2^32 - 1]");
    if (p->flags) return fail(ctx, KMU_E_BAD_ARG, "kmu_kfilter_params.flags must be 0");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    kmu_kfilter *f = new kmu_kfilter();
    f->ctx = ctx;
    f->p = *p;
    hipError_t e = hipMalloc((void **) &f->cells, p->n_cells * 16);
    if (e == hipSuccess) e = hipMalloc((void **) &f->scalars, 64);
    if (e != hipSuccess) {
        if (f->cells) (void) hipFree(f->cells);
        delete f;
        (void) hipGetLastError();
        return fail(ctx, KMU_E_OOM, "cannot allocate a prefilter of %llu cells", (unsigned long long) p->n_cells);
    }
    const int rc = kmu_kfilter_reset(f);
    if (rc != KMU_OK) {
        kmu_kfilter_destroy(f);
        return rc;
    }
    *out = f;
    return KMU_OK;
}

void kmu_kfilter_destroy(kmu_kfilter *f) {
    if (!f) return;
    (void) hipSetDevice(f->ctx->device);
    (void) hipStreamSynchronize(f->ctx->stream);
    if (f->cells) (void) hipFree(f->cells);
    if (f->scalars) (void) hipFree(f->scalars);
    delete f;
}

int kmu_kfilter_reset(kmu_kfilter *f) {
    if (!f) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KMU_HIP(ctx, hipMemsetAsync(f->cells, 0, f->p.n_cells * 16, ctx->stream));
    KMU_HIP(ctx, hipMemsetAsync(f->scalars, 0, 64, ctx->stream));
    return KMU_OK;
}

int kmu_kfilter_add_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem) {
    if (!f) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KfReads r;
    KMU_TRY(kf_stage(f, bases, offsets, n_seq, mem, &r));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    if (n_seq)
        KMU_TRY(launch(ctx, "k_kf_add_flat", k_kf_add_flat, dim3(ctx->num_cus * 8), dim3(256), 0, r.ds.bases, r.ds.offsets, n_seq, f->p.kmer_size,
                       view_of(f), f->scalars, d_err));
    return finish_checked(ctx, mem, d_err);
}

int kmu_kfilter_add_kmers(kmu_kfilter *f, const uint64_t *canon_kmers, uint64_t n, int mem) {
    if (!f || (!canon_kmers && n) || kf_bad_mem(mem)) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return KMU_OK;
    const uint64_t *d_k;
    KMU_TRY(stage_to_device(ctx, "kf.in.k", canon_kmers, n, mem, &d_k));
    KMU_TRY(launch(ctx, "k_kf_add_kmers", k_kf_add_kmers, dim3(grid_for(ctx, n, 256)), dim3(256), 0, d_k, n, view_of(f), f->scalars));
    return finish_call(ctx, mem);
}

int kmu_kfilter_query(kmu_kfilter *f, const uint64_t *canon_kmers, uint64_t n, int mem, uint8_t *class_out) {
    if (!f || ((!canon_kmers || !class_out) && n) || kf_bad_mem(mem)) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    if (n == 0) return KMU_OK;
    const uint64_t *d_k;
    KMU_TRY(stage_to_device(ctx, "kf.in.k", canon_kmers, n, mem, &d_k));
    uint8_t *d_o;
    KMU_TRY(place_output(ctx, "kf.out.c", class_out, n + 16, mem, &d_o));
    KMU_TRY(launch(ctx, "k_kf_query", k_kf_query, dim3(grid_for(ctx, n, 256)), dim3(256), 0, d_k, n, view_of(f), d_o));
    KMU_TRY(bring_output(ctx, class_out, d_o, n, mem));
    return finish_call(ctx, mem);
}

int kmu_kfilter_info(kmu_kfilter *f, kmu_kfilter_info_t *out) {
    if (!f || !out) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KMU_HIP(ctx, hipMemsetAsync(f->scalars + 1, 0, 16, ctx->stream));
    KMU_TRY(launch(ctx, "k_kf_popcount", k_kf_popcount, dim3(grid_for(ctx, f->p.n_cells, 1024)), dim3(256), 0, f->cells, f->p.n_cells, f->scalars));
    uint64_t h[3];
    KMU_TRY(read_back(ctx, {{h, f->scalars, sizeof h}}));
    out->n_cells = f->p.n_cells;
    out->bytes = f->p.n_cells * 16;
    out->n_hashes = f->p.n_hashes;
    out->kmer_size = (uint32_t) f->p.kmer_size;
    out->n_added = h[0];
    out->bits_a = h[1];
    out->bits_b = h[2];
    out->est_distinct = kf_est_distinct(f->p.n_cells, f->p.n_hashes, h[1]);
    return KMU_OK;
}

int kmu_kfilter_export(kmu_kfilter *f, uint64_t *words_out, int mem) {
    if (!f || !words_out || kf_bad_mem(mem)) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KMU_HIP(ctx, hipMemcpyAsync(words_out, f->cells, f->p.n_cells * 16, mem == KMU_MEM_HOST ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice,
                                ctx->stream));
    return finish_call(ctx, mem);
}

int kmu_kfilter_merge(kmu_kfilter *dst, const kmu_kfilter *src) {
    if (!dst || !src || dst == src) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = dst->ctx;
    if (src->ctx != ctx) return fail(ctx, KMU_E_BAD_ARG, "kmu_kfilter_merge: the two filters belong to different contexts");
    if (src->p.kmer_type != dst->p.kmer_type || src->p.kmer_size != dst->p.kmer_size || src->p.n_hashes != dst->p.n_hashes ||
        src->p.flags != dst->p.flags || src->p.n_cells != dst->p.n_cells)
        return fail(ctx, KMU_E_BAD_ARG, "kmu_kfilter_merge: the two filters differ in their parameters");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KMU_TRY(launch(ctx, "k_kf_merge", k_kf_merge, dim3(grid_for(ctx, dst->p.n_cells, 1024)), dim3(256), 0, dst->cells, (const uint64_t *) src->cells,
                   dst->p.n_cells, dst->scalars, (const uint64_t *) src->scalars));
    return finish_call(ctx, KMU_MEM_DEVICE);
}

int kmu_kfilter_select_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem, uint64_t *kmers_out,
                             uint64_t cap, uint64_t *n_out) {
    if (!f || !n_out) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = f->ctx;
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    if (n_seq == 0) return KMU_OK;
    KfReads r;
    KMU_TRY(kf_stage(f, bases, offsets, n_seq, mem, &r));
    if (r.total_bases == 0) return KMU_OK;
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    uint64_t *base, nsteps;
    int grid;
    KMU_TRY(kf_pass_scan(f, r, d_err, &base, &nsteps, &grid));
    uint64_t n = 0;
    // (not read_back: the copy of the error word goes between this copy and the one synchronisation, check_err_word's)
    KMU_HIP(ctx, hipMemcpyAsync(&n, base + nsteps, 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_TRY(check_err_word(ctx, d_err));
    *n_out = n;
    if (!kmers_out) return KMU_OK; // size query
    if (cap < n) return fail(ctx, KMU_E_BAD_ARG, "output too small: %llu k-mers", (unsigned long long) n);
    if (n == 0) return KMU_OK;
    uint64_t *d_k;
    KMU_TRY(place_output(ctx, "kf.ws", kmers_out, n + 8, mem, &d_k));
    KMU_TRY(launch(ctx, "k_kf_pass_emit", k_kf_pass_emit, dim3(grid), dim3(256), 0, r.ds.bases, r.ds.offsets, n_seq, f->p.kmer_size, view_of(f),
                   (const uint64_t *) base, (uint64_t) 0, nsteps, d_k));
    KMU_TRY(bring_output(ctx, kmers_out, d_k, n, mem));
    return finish_call(ctx, mem);
}

// The host driver of the filtered add: k_kf_pass_count and the scan once; the wave steps cut into consecutive ranges whose
// survivors fit a workspace of KMU_KFILTER_CHUNK_KMERS k-mers (default 2^26: 512 MiB); per range k_kf_pass_emit into the
// workspace, then add_entries -- the direct / partitioned choice and every count kernel as they are.
int kmu_count_add_reads_filtered(kmu_counter *c, kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                                 uint64_t *n_passed_out) {
    if (!c || !f) return KMU_E_BAD_ARG;
    kmu_ctx *ctx = c->ctx;
    if (n_passed_out) *n_passed_out = 0;
    if (f->ctx != ctx) return fail(ctx, KMU_E_BAD_ARG, "the counter and the prefilter belong to different contexts");
    if (c->p.kmer_type != f->p.kmer_type || c->p.kmer_size != f->p.kmer_size)
        return fail(ctx, KMU_E_BAD_ARG, "the counter and the prefilter differ in k-mer type or size");
    if (c->dist) return fail(ctx, KMU_E_UNSUPPORTED, "the filtered add takes a counter that is not distributed");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    KfReads r;
    KMU_TRY(kf_stage(f, bases, offsets, n_seq, mem, &r));
    if (n_seq == 0 || r.total_bases == 0) return KMU_OK;
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    uint64_t *base, nsteps;
    int grid;
    KMU_TRY(kf_pass_scan(f, r, d_err, &base, &nsteps, &grid));
    uint64_t cap = 1ull << 26;
    if (const char *e = getenv("KMU_KFILTER_CHUNK_KMERS")) cap = (uint64_t) std::max<long long>(atoll(e), 0);
    cap = std::max<uint64_t>(cap, 2048); // (a wave step holds up to 1024 k-mers; twice that bounds the number of ranges)
    const uint64_t max_ranges = r.total_bases / (cap - 1023) + 2;
    uint64_t *cut;
    KMU_TRY(dev_array(ctx, "kf.cut", 2 * (max_ranges + 1) + 1, &cut));
    uint64_t *d_nr = cut + 2 * (max_ranges + 1);
    KMU_TRY(launch(ctx, "k_kf_cut", k_kf_cut, dim3(1), dim3(64), 0, (const uint64_t *) base, nsteps, cap, max_ranges, cut, d_nr));
    std::vector<uint64_t> h_cut(2 * (max_ranges + 1) + 1);
    KMU_HIP(ctx, hipMemcpyAsync(h_cut.data(), cut, h_cut.size() * 8, hipMemcpyDeviceToHost, ctx->stream));
    KMU_TRY(check_err_word(ctx, d_err)); // (the one synchronisation: the ranges with the total, and what the walk found)
    const uint64_t n_ranges = h_cut.back();
    if (n_ranges > max_ranges || h_cut[2 * n_ranges] != nsteps) return fail(ctx, KMU_E_HIP, "kmu_count_add_reads_filtered: the ranges do not cover the reads");
    const uint64_t passed = h_cut[2 * n_ranges + 1];
    if (passed == 0) return KMU_OK;
    if (c->deferred) KMU_TRY(table_alloc_for(c, nullptr, 0, d_err, 0.0, std::max<uint64_t>(c->p.capacity_hint, passed))); // (for all ranges, not the first)
    uint64_t *ws;
    KMU_TRY(dev_array(ctx, "kf.ws", std::min(cap, passed) + 8, &ws));
    uint64_t done = 0;
    for (uint64_t i = 0; i < n_ranges; i++) {
        const uint64_t st_lo = h_cut[2 * i], st_hi = h_cut[2 * i + 2], n = h_cut[2 * i + 3] - h_cut[2 * i + 1];
        if (n == 0) continue;
        if (n > std::min(cap, passed)) return fail(ctx, KMU_E_HIP, "kmu_count_add_reads_filtered: a range beyond the workspace");
        KMU_TRY(launch(ctx, "k_kf_pass_emit", k_kf_pass_emit, dim3(grid_for(ctx, st_hi - st_lo, 4)), dim3(256), 0, r.ds.bases, r.ds.offsets, n_seq,
                       f->p.kmer_size, view_of(f), (const uint64_t *) base, st_lo, st_hi, ws));
        KMU_TRY(add_entries(c, ws, nullptr, n, KMU_MEM_DEVICE));
        done += n;
        if (n_passed_out) *n_passed_out = done;
    }
    return finish_call(ctx, mem);
}

} // extern "C"

// kmu_sketch_dens.hip -- one-permutation hashing with optimal / reverse-optimal densification for gfx950.
//
// Reference loop (src/sketching/setsketchert.rs:385-463, 521-599; AA: src/aautils/setsketchert.rs:482-746): for every
// k-mer occurrence `sminhash.sketch(&fhash(kmer))`, then `end_sketch()` ("it calls densification!"), then `get_hsketch()`.
// `sketch`: seed an RNG from hasher(value), draw r in [0,1) and a bin k in [0,m); bin k keeps its smallest r.
// `end_sketch`: bins no item fell into are filled from bins that were -- OptDens: an empty bin probes h(i, attempt) until
// it meets a filled one (Shrivastava 2017); RevOptDens: in rounds, every filled bin offers itself to bin h(j, round), an
// empty bin takes the smallest j (Mai et al. 2019).  (Inner arithmetic: crate probminhash::densminhash, not in the
// reference tree -- "parity unpinned", DESIGN.md section 5 says what is restated and what is this implementation's.)
//
// Device mapping.  The sketch is a per-bin minimum over items, so items are independent: one lane per k-mer occurrence,
// `ds_min_u64` on the order-preserving bit pattern of the (positive) value; no multiset, no staging.
//   k_oph_reads<false>  one 256-thread workgroup per sequence (queue), bins in LDS, densification in LDS, row out
//   k_oph_reads<true>   one signature for all sequences: every workgroup accumulates the sequences it takes, then merges
//                       its bins into one global row (atomicMin)
//   k_oph_long          a sequence too long for one workgroup (genomes): the whole grid walks its words, same merge
//   k_oph_finish        one workgroup: global row -> LDS -> densify -> signature row
// Densification in parallel, same result as the sequential statement: the "filled by an item" bitmap is fixed before it
// starts, so an OptDens bin's search does not depend on the order bins are visited in; a RevOptDens round resolves
// competing offers with an atomic minimum on the offering bin's index.
#include <algorithm>
#include <vector>

#include "kmu_sketch_dens.h"

namespace kmu {

template <bool ALL, bool HLL>
__global__ void __launch_bounds__(256) k_oph_reads(DensArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *hs;
    uint32_t *filled, *cnt, *claim;
    oph_lds(a, smem, hs, filled, cnt, claim);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid >> 6, nwaves = nthreads >> 6;
    const bool aa = a.cfg.kmer_type == KMU_KMERAA32BIT || a.cfg.kmer_type == KMU_KMERAA64BIT;
    const uint64_t large = oph_neutral(a);
    for (int s = tid; s < a.m; s += nthreads) {
        hs[s] = large;
        if (a.rev && !ALL) claim[s] = 0xFFFFFFFFu;
    }
    if (tid == 0) { cnt[2] = atomicAdd(a.queue, 1u); cnt[3] = 0; } // cnt[3]: K_low of the registers (SetSketch)
    __syncthreads();
    for (;;) {
        const uint32_t r = cnt[2];
        __syncthreads(); // everyone holds r before thread 0 posts the next one
        if (r >= a.n_seq) break;
        uint32_t r_next = 0;
        if (tid == 0) r_next = atomicAdd(a.queue, 1u);
        const SeqView sv = dens_view(a, r);
        const uint64_t L = sv.len;
        const uint64_t nk = L >= (uint64_t) a.cfg.k ? L - a.cfg.k + 1 : 0;
        if (L == 0 && tid == 0 && !a.hashed_bytes) atomicOr(a.err, 8u);
        const bool skip = a.skip_longer && nk > (uint64_t) a.skip_longer; // k_oph_long's
        if (!skip) {
            uint32_t bad = 0;
            if (nk == 0 && !a.hashed_bytes) bad = wave_validate_seq(sv, wave, nwaves, aa);
            else bad = oph_walk<HLL>(a, sv, hs, &cnt[3], aa, nk, (uint64_t) wave, (uint64_t) nwaves);
            if (bad) atomicOr(a.err, aa ? DERR_BAD_AA : DERR_NON_ACGT);
        }
        __syncthreads();
        if (!ALL && !skip) {
            if (!a.hll) oph_densify(a, hs, filled, claim, cnt);
            oph_store_row(a, hs, (uint64_t) r);
            __syncthreads();
            for (int s = tid; s < a.m; s += nthreads) hs[s] = large;
            if (tid == 0) cnt[3] = 0;
        }
        if (tid == 0) cnt[2] = r_next;
        __syncthreads();
    }
    if (ALL) oph_merge_to_row(a, hs);
}

// one long sequence, walked by the whole grid; bins merged into a.row
template <bool HLL>
__global__ void __launch_bounds__(256) k_oph_long(DensArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *hs = reinterpret_cast<uint64_t *>(smem);
    uint32_t *klow = reinterpret_cast<uint32_t *>(hs + a.m);
    const int tid = threadIdx.x, nthreads = blockDim.x;
    const int wave = tid >> 6, nwaves = nthreads >> 6;
    const bool aa = a.cfg.kmer_type == KMU_KMERAA32BIT || a.cfg.kmer_type == KMU_KMERAA64BIT;
    const uint64_t large = oph_neutral(a);
    for (int s = tid; s < a.m; s += nthreads) hs[s] = large;
    if (tid == 0) *klow = 0;
    __syncthreads();
    const SeqView sv = dens_view(a, a.long_seq);
    const uint64_t nk = sv.len >= (uint64_t) a.cfg.k ? sv.len - a.cfg.k + 1 : 0;
    const uint32_t bad = oph_walk<HLL>(a, sv, hs, klow, aa, nk, (uint64_t) blockIdx.x * nwaves + wave, (uint64_t) gridDim.x * nwaves);
    if (bad) atomicOr(a.err, aa ? DERR_BAD_AA : DERR_NON_ACGT);
    __syncthreads();
    oph_merge_to_row(a, hs);
}

__global__ void __launch_bounds__(256) k_oph_fill(uint64_t *row, int m, uint64_t bits) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t < m) row[t] = bits;
}

// global row -> densified signature row a.out_row
__global__ void __launch_bounds__(256) k_oph_finish(DensArgs a) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint64_t *hs;
    uint32_t *filled, *cnt, *claim;
    oph_lds(a, smem, hs, filled, cnt, claim);
    for (int s = threadIdx.x; s < a.m; s += blockDim.x) {
        hs[s] = a.row[s];
        if (a.rev) claim[s] = 0xFFFFFFFFu;
    }
    __syncthreads();
    if (!a.hll) oph_densify(a, hs, filled, claim, cnt);
    oph_store_row(a, hs, a.out_row);
}

__global__ void __launch_bounds__(1024) k_dens_max_len(const uint64_t *offsets, uint32_t n_seq, uint64_t *out) {
    uint64_t mx = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += gridDim.x * blockDim.x) {
        const uint64_t L = offsets[i + 1] - offsets[i];
        mx = L > mx ? L : mx;
    }
    mx = wave_max_u64(mx);
    if (lane_id() == 0 && mx) atomicMax((unsigned long long *) out, (unsigned long long) mx);
}

static constexpr uint32_t DENS_LONG_KMERS = 1u << 20; // longer sequences are spread over the grid

// kmu_log on the host (for 1 / ln b): the same operations in the same order
static double host_log(double x) {
    uint64_t bits;
    memcpy(&bits, &x, 8);
    int e = (int) ((bits >> 52) & 0x7FF) - 1023;
    bits = (bits & 0x000FFFFFFFFFFFFFull) | 0x3FF0000000000000ull;
    double f;
    memcpy(&f, &bits, 8);
    if (f > 1.4142135623730951) { f = f * 0.5; e += 1; }
    const double s = (f - 1.0) / (f + 1.0), z = s * s;
    double poly = 1.0 / 21.0;
    poly = poly * z + 1.0 / 19.0;
    poly = poly * z + 1.0 / 17.0;
    poly = poly * z + 1.0 / 15.0;
    poly = poly * z + 1.0 / 13.0;
    poly = poly * z + 1.0 / 11.0;
    poly = poly * z + 1.0 / 9.0;
    poly = poly * z + 1.0 / 7.0;
    poly = poly * z + 1.0 / 5.0;
    poly = poly * z + 1.0 / 3.0;
    poly = poly * z + 1.0;
    return (double) e * 0.6931471805599453 + 2.0 * s * poly;
}

void dens_args(const kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const void *hashed,
               int hashed_bytes, DensArgs *out) {
    DensArgs &a = *out;
    memset(&a, 0, sizeof a);
    a.hashed = hashed;
    a.hashed_bytes = hashed_bytes;
    a.bases = ds.bases;
    a.offsets = ds.offsets;
    a.packed_offsets = ds.packed_offsets;
    a.n_seq = ds.n_seq;
    a.packed = ds.packed;
    a.total_bytes = ds.total_bytes;
    a.cfg = KmerCfg{p->kmer_type, hashed_bytes ? 1 : p->kmer_size, p->fhash};
    a.m = p->sketch_size;
    a.hasher = p->hasher;
    a.rand08 = (p->flags & KMU_FLAG_RAND08) ? 1 : 0;
    a.f32 = p->sig_type == KMU_SIG_F32;
    a.val_w32 = kmer_val_bytes(p->kmer_type) == 4;
    a.rev = p->algo == KMU_ALGO_REVOPTDENS;
    a.hll = p->algo == KMU_ALGO_HLL;
    a.sig_bytes = (int) sig_elem_bytes(p->sig_type);
    a.idx_thresh = (0u - (uint32_t) a.m) % (uint32_t) a.m;
    a.idx_zone = 0xFFFFFFFFFFFFFFFFull - (0xFFFFFFFFFFFFFFFFull - (uint64_t) a.m + 1ull) % (uint64_t) a.m;
    if (a.hll) { // SetSketchParams of the context; 1 / ln b with the kernels' own logarithm (same formula on the host)
        a.q = ctx->hll.q;
        a.inv_am = 1.0 / (ctx->hll.a * (double) a.m);
        a.inv_ln_b = 1.0 / host_log(ctx->hll.b);
    }
    a.sig_out = d_sig;
    a.err = d_err;
}

int dens_lds_check(kmu_ctx *ctx, const DensArgs &a, const void *const *fns, int n_fns) {
    const size_t lds_full = dens_lds_full(a);
    if (lds_full > DENS_LDS_MAX)
        return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %d: the bins of a densified sketch (%zu B) do not fit the LDS", a.m, lds_full);
    if (lds_full > 64 * 1024)
        for (int i = 0; i < n_fns; i++)
            if (hipFuncSetAttribute(fns[i], hipFuncAttributeMaxDynamicSharedMemorySize, (int) DENS_LDS_MAX) != hipSuccess) {
                (void) hipGetLastError();
                return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %d needs %zu B of LDS", a.m, lds_full);
            }
    return KMU_OK;
}

// OptDens / RevOptDens for every mode of kmu_sketch / kmu_sketch_hashed
int launch_dens(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, void *d_sig, uint32_t *d_err, const void *hashed,
                int hashed_bytes) {
    DensArgs a;
    dens_args(ctx, p, ds, d_sig, d_err, hashed, hashed_bytes, &a);
    const bool all = p->mode == KMU_MODE_ALL_SEQS;
    const size_t lds_acc = (size_t) 8 * a.m + 16; // bins only (k_oph_long)
    const size_t lds_full = dens_lds_full(a), lds_max = DENS_LDS_MAX;
    const void *fns[7] = {(const void *) k_oph_reads<false, false>, (const void *) k_oph_reads<true, false>,
                          (const void *) k_oph_reads<false, true>,  (const void *) k_oph_reads<true, true>,
                          (const void *) k_oph_long<false>,         (const void *) k_oph_long<true>,
                          (const void *) k_oph_finish};
    KMU_TRY(dens_lds_check(ctx, a, fns, 7));
    uint64_t *row;
    void *q, *mx;
    KMU_TRY(dev_buf(ctx, "queue", 64, &q));
    KMU_HIP(ctx, hipMemsetAsync(q, 0, 64, ctx->stream));
    a.queue = (uint32_t *) q;
    KMU_TRY(dev_array(ctx, "dens.row", (size_t) a.m + 8, &row));
    a.row = row;
    const uint64_t large = dens_neutral_bits(a);
    auto fill_row = [&]() { return launch(ctx, nullptr, k_oph_fill, dim3((a.m + 255) / 256), dim3(256), 0, a.row, a.m, large); };
    // sequences too long for one workgroup: found on the host from the offsets (only if the longest one calls for it)
    std::vector<uint32_t> long_seqs;
    if (ds.n_seq) {
        KMU_TRY(dev_buf(ctx, "pmh.maxlen", 64, &mx));
        KMU_HIP(ctx, hipMemsetAsync(mx, 0, 8, ctx->stream));
        const uint32_t mgrid = (uint32_t) std::min<uint64_t>(((uint64_t) ds.n_seq + 1023) / 1024, (uint64_t) ctx->num_cus);
        KMU_TRY(launch(ctx, nullptr, k_dens_max_len, dim3(mgrid ? mgrid : 1), dim3(1024), 0, ds.offsets, ds.n_seq, (uint64_t *) mx));
        uint64_t max_len = 0;
        KMU_TRY(read_back(ctx, {{&max_len, mx, 8}}));
        if (max_len > (uint64_t) DENS_LONG_KMERS + (uint64_t) a.cfg.k) {
            std::vector<uint64_t> h_off((size_t) ds.n_seq + 1);
            KMU_HIP(ctx, hipMemcpyAsync(h_off.data(), ds.offsets, ((size_t) ds.n_seq + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
            KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
            for (uint32_t i = 0; i < ds.n_seq; i++) {
                const uint64_t L = h_off[i + 1] - h_off[i];
                if (L >= (uint64_t) a.cfg.k && L - a.cfg.k + 1 > DENS_LONG_KMERS) long_seqs.push_back(i);
            }
            a.skip_longer = DENS_LONG_KMERS;
        }
    }
    const int per_cu = (int) std::max<size_t>(1, std::min<size_t>(8, lds_max / lds_full));
    const int grid = grid_for(ctx, ds.n_seq, 1, per_cu);
    if (all) KMU_TRY(fill_row());
    const auto reads = all ? (a.hll ? k_oph_reads<true, true> : k_oph_reads<true, false>) : (a.hll ? k_oph_reads<false, true> : k_oph_reads<false, false>);
    KMU_TRY(launch(ctx, "k_oph_reads", reads, dim3(grid), dim3(256), lds_full, a));
    const int grid_long = ctx->num_cus * (int) std::max<size_t>(1, std::min<size_t>(8, lds_max / std::max<size_t>(lds_acc, 1024)));
    for (uint32_t i : long_seqs) {
        if (!all) KMU_TRY(fill_row());
        a.long_seq = i;
        KernelTimer t(ctx, "k_oph_long"); // (with the finish of the sequence's own row)
        KMU_TRY(launch(ctx, nullptr, a.hll ? k_oph_long<true> : k_oph_long<false>, dim3(grid_long), dim3(256), lds_acc, a));
        if (!all) {
            a.out_row = i;
            KMU_TRY(launch(ctx, nullptr, k_oph_finish, dim3(1), dim3(256), lds_full, a));
        }
    }
    if (all && ctx->partial_out) { // the bins before densification are what other ranks' bins are merged with
        KMU_HIP(ctx, hipMemcpyAsync(ctx->partial_out, a.row, (size_t) 8 * a.m, hipMemcpyDeviceToDevice, ctx->stream));
    } else if (all) {
        a.out_row = 0;
        KMU_TRY(launch(ctx, "k_oph_finish", k_oph_finish, dim3(1), dim3(256), lds_full, a));
    }
    return KMU_OK;
}

__global__ void __launch_bounds__(256) k_oph_merge(const uint64_t *parts, uint32_t n_parts, int m, int take_max, uint64_t *row) {
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= m) return;
    uint64_t best = parts[t];
    for (uint32_t i = 1; i < n_parts; i++) {
        const uint64_t v = parts[(uint64_t) i * m + t];
        best = (take_max ? v > best : v < best) ? v : best;
    }
    row[t] = best;
}

// bins of several ranks (device memory, n_parts x m patterns) -> one densified signature row
int launch_dens_merge(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *parts, uint32_t n_parts, void *d_sig) {
    DensArgs a;
    memset(&a, 0, sizeof a);
    a.m = p->sketch_size;
    a.f32 = p->sig_type == KMU_SIG_F32;
    a.rev = p->algo == KMU_ALGO_REVOPTDENS;
    a.hll = p->algo == KMU_ALGO_HLL;
    a.sig_bytes = (int) sig_elem_bytes(p->sig_type);
    a.sig_out = d_sig;
    const size_t lds_full = ((size_t) 8 * a.m + 4 * ((size_t) (a.m + 31) / 32) + 16 + (a.rev ? (size_t) 4 * a.m : 0) + 15) & ~(size_t) 15;
    if (lds_full > 160 * 1024) return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %d: the bins do not fit the LDS", a.m);
    if (lds_full > 64 * 1024 &&
        hipFuncSetAttribute((const void *) k_oph_finish, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024) != hipSuccess) {
        (void) hipGetLastError();
        return fail(ctx, KMU_E_UNSUPPORTED, "sketch_size %d needs %zu B of LDS", a.m, lds_full);
    }
    uint64_t *row;
    KMU_TRY(dev_array(ctx, "dens.row", (size_t) a.m + 8, &row));
    a.row = row;
    KMU_TRY(launch(ctx, nullptr, k_oph_merge, dim3((a.m + 255) / 256), dim3(256), 0, parts, n_parts, a.m, a.hll, a.row));
    a.out_row = 0;
    return launch(ctx, nullptr, k_oph_finish, dim3(1), dim3(256), lds_full, a);
}

} // namespace kmu

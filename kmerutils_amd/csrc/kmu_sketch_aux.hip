// kmu_sketch_aux.hip -- the small kernels around the sketch routes: longest sequence, k-mer count scan, compact hashing, widening.
#include "kmu_sketch_kernels.h"
#include "kmu_stream.h"

namespace kmu {

// longest sequence: out[0] = max_i (offsets[i + 1] - offsets[i]); out[0] must be 0 on entry.  out[1] = sum of the lengths
__global__ void __launch_bounds__(1024) k_max_len(const uint64_t *offsets, uint32_t n_seq, uint64_t *out) {
    uint64_t mx = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_seq; i += gridDim.x * blockDim.x) {
        const uint64_t L = offsets[i + 1] - offsets[i];
        mx = L > mx ? L : mx;
    }
    mx = wave_max_u64(mx);
    if (lane_id() == 0 && mx) atomicMax((unsigned long long *) out, (unsigned long long) mx);
    if (blockIdx.x == 0 && threadIdx.x == 0) out[1] = offsets[n_seq] - offsets[0]; // all bases of the call
}

// exclusive scan of the k-mer counts max(0, L_i - k + 1) of all sequences (single workgroup); koff[n] = total
__global__ void __launch_bounds__(1024) k_nk_scan(const uint64_t *offsets, uint32_t n_seq, int k, uint64_t *koff,
                                                  uint32_t *err) {
    __shared__ uint64_t wtot[16];
    __shared__ uint64_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t base = 0; base < n_seq; base += blockDim.x) {
        const uint32_t i = base + threadIdx.x;
        uint64_t v = 0;
        if (i < n_seq) {
            const uint64_t L = offsets[i + 1] - offsets[i];
            if (L == 0) atomicOr(err, 8u);
            v = L >= (uint64_t) k ? L - k + 1 : 0;
        }
        uint64_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t o = ((uint64_t) (uint32_t) __shfl_up((int) (incl >> 32), d, 64) << 32) |
                         (uint32_t) __shfl_up((int) (uint32_t) incl, d, 64);
            if (lane_id() >= d) incl += o;
        }
        if (lane_id() == 63) wtot[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint64_t pre = carry;
        for (int w = 0; w < (int) (threadIdx.x >> 6); w++) pre += wtot[w];
        if (i < n_seq) koff[i] = pre + incl - v;
        __syncthreads();
        if (threadIdx.x == blockDim.x - 1) carry = pre + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) koff[n_seq] = carry;
}

// fhash(kmer) of every k-mer of every sequence, compact: out[koff[i] + p]
__global__ void __launch_bounds__(256) k_seq_hashes_compact(const uint8_t *bases, const uint64_t *offsets,
                                                            const uint64_t *packed_offsets, uint32_t n_seq, int packed,
                                                            uint64_t total, KmerCfg cfg, const uint64_t *koff, uint64_t *out,
                                                            uint32_t *err, int spread) {
    // spread = 0: one workgroup per sequence (many sequences); spread = 1: every sequence is walked by the whole grid
    // (a few long sequences, e.g. the contigs of a genome)
    const int wave = spread ? (int) (blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6)) : (int) (threadIdx.x >> 6);
    const int nwaves = spread ? (int) (gridDim.x * (blockDim.x >> 6)) : (int) (blockDim.x >> 6);
    const bool aa = cfg.kmer_type == KMU_KMERAA32BIT || cfg.kmer_type == KMU_KMERAA64BIT;
    for (uint32_t i = spread ? 0u : blockIdx.x; i < n_seq; i += spread ? 1u : gridDim.x) {
        SeqView s;
        s.base = bases;
        s.len = offsets[i + 1] - offsets[i];
        s.packed = packed;
        if (packed) {
            s.begin = packed_offsets[i];
            s.total = total ? total : (packed_offsets[n_seq - 1] + (offsets[n_seq] - offsets[n_seq - 1] + 3) / 4);
        } else {
            s.begin = offsets[i];
            s.total = total ? total : offsets[n_seq];
        }
        const uint64_t nk = s.len >= (uint64_t) cfg.k ? s.len - cfg.k + 1 : 0;
        uint64_t *o = out + koff[i];
        uint32_t bad = 0;
        if (nk == 0) bad |= wave_validate_seq(s, wave, nwaves, aa);
        else if (aa) {
            for (uint64_t st = wave; st < (s.len + 63) / 64; st += nwaves)
                bad |= wave_step_kmers_aa(s, cfg.k, st, 0, nk, [&](uint64_t p, uint64_t val, uint64_t) { o[p] = apply_fhash(cfg, val, 0); });
        } else {
            for (uint64_t st = wave; st < (seq_num_words(s) + 63) / 64; st += nwaves)
                bad |= wave_step_kmers(s, cfg.k, st, 0, nk, [&](uint64_t p, uint64_t val, uint64_t rc) { o[p] = apply_fhash(cfg, val, rc); });
        }
        if (bad) atomicOr(err, aa ? DERR_BAD_AA : DERR_NON_ACGT);
    }
}

__global__ void __launch_bounds__(256) k_widen_u32(const uint32_t *in, uint64_t n, uint64_t *out) {
    for (uint64_t i = (uint64_t) blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t) gridDim.x * blockDim.x) out[i] = in[i];
}

} // namespace kmu

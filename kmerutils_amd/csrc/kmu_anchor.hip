// kmu_anchor.hip -- read anchors: one bottom-k row (hashes, multiplicities) per overlapping window of every read
// (kmu_anchor_layout / kmu_read_anchors; ReadAnchors, src/anchor.rs:228-329, over MinInvHashCountKmer, minhash.rs:204-289).
//
// k_read_anchors: one launch for all rows of a call, one wave (a 64-thread workgroup) per row, rows dealt grid-stride.
//  - row -> read by a 64-ary search in anchor_row_offsets (wave_find_read); slice s = row - first row of the read starts at
//    beg = s * stride and ends at min(beg + window, L - 1).  The slice is walked as a SeqView over the batch's base array:
//    nothing is copied per window, and wave_step_kmers keeps the k-mers that lie wholly inside it.
//  - selection in tiles of KMU_ANCHOR_TILE_KMERS k-mers: the hashes of a tile go into LDS as (hash, 1) pairs behind the carry
//    list -- the <= nbkmer smallest (hash, count) pairs so far --, the whole is sorted (bitonic, padded to a power of two with
//    (u64::MAX, 0)) and runs of equal hashes collapse into (hash, sum of counts): the first nbkmer of them are the next carry.
//    TILE + MAX_NBKMER = 1024 = the largest sort.  A hash of the final list is in every intermediate list (a hash that leaves
//    one is larger than nbkmer others for good), so its count is its total multiplicity; it is masked at the end as
//    kmu_sketch masks it (u8 counts under KMU_HASHER_INT64HASH, u16 otherwise: both wrap upstream).
//  LDS: 8 KiB hashes + 4 KiB counts + 3 KiB for the collapsed list = 15 KiB per one-wave workgroup (ten per CU).
#include <algorithm>

#include "kmu_flat.h"
#include "kmu_sketch_host.hpp"
#include "kmu_stream.h"

namespace kmu {

static constexpr uint32_t ANCHOR_SORT_MAX = KMU_ANCHOR_TILE_KMERS + KMU_ANCHOR_MAX_NBKMER;
static_assert((ANCHOR_SORT_MAX & (ANCHOR_SORT_MAX - 1)) == 0, "tile + carry must fill a power-of-two sort");

struct AnchorArgs {
    const uint8_t *bases;
    const uint64_t *offsets;  // n_seq + 1
    const uint64_t *row_off;  // n_seq + 1: first row of every read
    uint32_t n_seq;
    uint32_t rows;
    uint64_t total_bytes;     // size of `bases`, or 0: offsets[n_seq]
    uint32_t window, stride;
    KmerCfg cfg;
    uint32_t m;               // nbkmer
    int hasher;
    uint32_t count_mask;
    uint64_t *hashes_out;
    uint32_t *counts_out;     // may be null
    uint32_t *n_out;          // may be null
    uint32_t *err;
};

__global__ void __launch_bounds__(64) k_read_anchors(AnchorArgs a) {
    __shared__ uint64_t keys[ANCHOR_SORT_MAX];
    __shared__ uint32_t cnts[ANCHOR_SORT_MAX];
    __shared__ uint64_t outk[KMU_ANCHOR_MAX_NBKMER];
    __shared__ uint32_t start[KMU_ANCHOR_MAX_NBKMER + 1];
    const uint32_t lane = (uint32_t) lane_id();
    const uint32_t m = a.m;
    const int k = a.cfg.k;
    const bool w32 = is_u32_type(a.cfg.kmer_type);
    const uint64_t total = a.total_bytes ? a.total_bytes : a.offsets[a.n_seq];
    uint32_t bad = 0;
    for (uint32_t row = blockIdx.x; row < a.rows; row += gridDim.x) {
        const uint32_t r = wave_find_read(a.row_off, a.n_seq, (uint64_t) row);
        const uint64_t rbeg = a.offsets[r], L = a.offsets[r + 1] - rbeg;
        const uint64_t beg = (uint64_t) (row - a.row_off[r]) * a.stride;
        uint32_t cn = 0; // entries of the carry list: keys[0 .. cn), cnts[0 .. cn)
        if (beg < L) {   // (always, with the row offsets of kmu_anchor_layout)
            const uint64_t end = std::min<uint64_t>(beg + a.window, L - 1);
            SeqView s;
            s.base = a.bases; s.begin = rbeg + beg; s.len = end - beg; s.total = total; s.packed = 0;
            const uint64_t nk = s.len >= (uint64_t) k ? s.len - k + 1 : 0;
            const uint64_t lead = seq_lead(s);
            if (nk == 0) bad |= wave_validate_seq(s, 0, 1, false);
            // the last slice of a read ends one base short of it: that base is checked here
            if (beg + a.stride >= L && lane == 0) bad |= !is_acgt(a.bases[rbeg + L - 1]);
            for (uint64_t t0 = 0; t0 < nk; t0 += KMU_ANCHOR_TILE_KMERS) {
                const uint64_t t1 = std::min<uint64_t>(t0 + KMU_ANCHOR_TILE_KMERS, nk);
                const uint32_t n_real = cn + (uint32_t) (t1 - t0);
                uint32_t N = 64;
                while (N < n_real) N <<= 1;
                for (uint64_t st = (t0 + lead) / 1024; st <= (t1 - 1 + lead) / 1024; st++)
                    bad |= wave_step_kmers(s, k, st, t0, t1, [&](uint64_t p, uint64_t val, uint64_t rc) {
                        const uint32_t i = cn + (uint32_t) (p - t0);
                        keys[i] = hasher_finish(a.hasher, apply_fhash(a.cfg, val, rc), w32);
                        cnts[i] = 1u;
                    });
                for (uint32_t i = n_real + lane; i < N; i += 64) {
                    keys[i] = 0xFFFFFFFFFFFFFFFFull;
                    cnts[i] = 0u;
                }
                __syncthreads();
                // bitonic sort of (hash, count) by hash, ascending
                for (uint32_t k2 = 2; k2 <= N; k2 <<= 1)
                    for (uint32_t j = k2 >> 1; j > 0; j >>= 1) {
                        for (uint32_t i = lane; i < N / 2; i += 64) {
                            const uint32_t lo = ((i & ~(j - 1)) << 1) | (i & (j - 1)), hi = lo | j;
                            const bool up = (lo & k2) == 0;
                            const uint64_t x = keys[lo], y = keys[hi];
                            if ((x > y) == up) {
                                const uint32_t cx = cnts[lo], cy = cnts[hi];
                                keys[lo] = y; keys[hi] = x;
                                cnts[lo] = cy; cnts[hi] = cx;
                            }
                        }
                        __syncthreads();
                    }
                // runs of equal hashes -> (hash, sum of counts): a lane takes N / 64 consecutive entries; the rank of a run and
                // the counts in front of it come from two wave scans
                const uint32_t ch = N / 64, i0 = lane * ch;
                uint32_t h = 0, sum = 0;
                for (uint32_t c = 0; c < ch; c++) {
                    const uint32_t i = i0 + c;
                    h += i < n_real && (i == 0 || keys[i - 1] != keys[i]);
                    sum += cnts[i];
                }
                const uint32_t hs = wave_incl_scan_u32(h), ss = wave_incl_scan_u32(sum);
                const uint32_t D = bcast_u32(hs, 63), all = bcast_u32(ss, 63);
                uint32_t rank = hs - h, before = ss - sum;
                for (uint32_t c = 0; c < ch; c++) {
                    const uint32_t i = i0 + c;
                    if (i < n_real && (i == 0 || keys[i - 1] != keys[i])) {
                        if (rank < m) outk[rank] = keys[i];
                        if (rank <= m) start[rank] = before;
                        rank++;
                    }
                    before += cnts[i];
                }
                if (lane == 0 && D <= m) start[D] = all;
                __syncthreads();
                cn = D < m ? D : m;
                for (uint32_t t = lane; t < cn; t += 64) {
                    keys[t] = outk[t];
                    cnts[t] = start[t + 1] - start[t];
                }
                __syncthreads();
            }
        }
        // the row: ascending hashes padded with u64::MAX, counts wrapped like the reference's (0 for padding)
        for (uint32_t t = lane; t < m; t += 64) {
            const bool have = t < cn;
            a.hashes_out[(uint64_t) row * m + t] = have ? keys[t] : 0xFFFFFFFFFFFFFFFFull;
            if (a.counts_out) a.counts_out[(uint64_t) row * m + t] = have ? (cnts[t] & a.count_mask) : 0u;
        }
        if (a.n_out && lane == 0) a.n_out[row] = cn;
        __syncthreads(); // the next row's tile overwrites the list
    }
    if (bad) atomicOr(a.err, DERR_NON_ACGT);
}

} // namespace kmu

using namespace kmu;

static bool anchor_shape_ok(uint32_t window, uint32_t overlap) { return window > 0 && window > overlap; } // anchor.rs:295-296

extern "C" int kmu_anchor_layout(const uint64_t *offsets, uint32_t n_seq, uint32_t window, uint32_t overlap, uint64_t *out) {
    if (!offsets || !out || !anchor_shape_ok(window, overlap)) return KMU_E_BAD_ARG;
    const uint64_t stride = window - overlap;
    out[0] = 0;
    for (uint32_t i = 0; i < n_seq; i++) {
        const uint64_t L = offsets[i + 1] - offsets[i];
        out[i + 1] = out[i] + (L + stride - 1) / stride; // one slice per beg = s * stride < L, anchor.rs:307-318
    }
    return KMU_OK;
}

extern "C" int kmu_read_anchors(kmu_ctx *ctx, const kmu_sketch_params *p_in, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                uint32_t window, uint32_t overlap, const uint64_t *anchor_row_offsets, uint64_t *hashes_out,
                                uint32_t *counts_out, uint32_t *n_out) {
    if (!ctx || !p_in) return KMU_E_BAD_ARG;
    if (!anchor_shape_ok(window, overlap))
        return fail(ctx, KMU_E_BAD_ARG, "anchors need window > 0 and window > overlap (anchor.rs:295-296), got %u / %u", window, overlap);
    if (p_in->algo != KMU_ALGO_BOTTOMK || p_in->block_size != 0)
        return fail(ctx, KMU_E_BAD_ARG, "read anchors are bottom-k rows (KMU_ALGO_BOTTOMK, block_size 0)");
    if (kmer_is_aa(p_in->kmer_type)) return fail(ctx, KMU_E_BAD_ALPHABET, "read anchors are defined on DNA k-mers");
    if (p_in->input_kind == KMU_INPUT_PACKED2) return fail(ctx, KMU_E_UNSUPPORTED, "read anchors take unpacked (ASCII) bases");
    if (p_in->sketch_size > KMU_ANCHOR_MAX_NBKMER)
        return fail(ctx, KMU_E_UNSUPPORTED, "nbkmer %d above KMU_ANCHOR_MAX_NBKMER (%d)", p_in->sketch_size, KMU_ANCHOR_MAX_NBKMER);
    kmu_sketch_params p_mode = *p_in, p_res;
    p_mode.mode = KMU_MODE_PER_SEQ;
    KMU_TRY(sketch_seq_params(ctx, &p_mode, p_mode.input_kind, &p_res));
    const kmu_sketch_params *p = &p_res;
    if (n_seq == 0) return KMU_OK;
    if (!offsets || !bases || !anchor_row_offsets) return fail(ctx, KMU_E_BAD_ARG, "null sequence buffers or anchor_row_offsets");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    uint64_t rows = 0;
    if (p->mem == KMU_MEM_HOST) {
        std::vector<uint64_t> want((size_t) n_seq + 1);
        (void) kmu_anchor_layout(offsets, n_seq, window, overlap, want.data());
        if (!std::equal(want.begin(), want.end(), anchor_row_offsets))
            return fail(ctx, KMU_E_BAD_ARG, "anchor_row_offsets is not the layout of kmu_anchor_layout for these reads");
        rows = want[n_seq];
    } else if (p->mem == KMU_MEM_DEVICE) KMU_TRY(read_back(ctx, {{&rows, anchor_row_offsets + n_seq}}));
    if (rows > 0xFFFFFFFFull) return fail(ctx, KMU_E_UNSUPPORTED, "%llu anchor rows: more than 2^32 - 1", (unsigned long long) rows);
    if (rows == 0) return KMU_OK;
    if (!hashes_out) return fail(ctx, KMU_E_BAD_ARG, "null hashes_out");
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, nullptr, n_seq, KMU_INPUT_ASCII, p->mem, &ds));
    const size_t m = (size_t) p->sketch_size;
    AnchorArgs a;
    a.bases = ds.bases;
    a.offsets = ds.offsets;
    a.n_seq = n_seq;
    a.rows = (uint32_t) rows;
    a.total_bytes = ds.total_bytes;
    a.window = window;
    a.stride = window - overlap;
    a.cfg = KmerCfg{p->kmer_type, p->kmer_size, p->fhash};
    a.m = (uint32_t) m;
    a.hasher = p->hasher;
    a.count_mask = p->hasher == KMU_HASHER_INT64HASH ? 0xFFu : 0xFFFFu; // MinInvHashCountKmer: u8, MinHashCount: u16
    KMU_TRY(stage_to_device(ctx, "in.anchorrows", anchor_row_offsets, (size_t) n_seq + 1, p->mem, &a.row_off));
    KMU_TRY(place_output(ctx, "out.sig", hashes_out, rows * m + 8, p->mem, &a.hashes_out));
    KMU_TRY(place_output(ctx, "out.counts", counts_out, rows * m + 16, p->mem, &a.counts_out));
    KMU_TRY(place_output(ctx, "out.anchor_n", n_out, rows + 16, p->mem, &a.n_out));
    KMU_TRY(get_err_word(ctx, &a.err));
    const uint32_t grid = (uint32_t) std::min<uint64_t>(rows, (uint64_t) ctx->num_cus * 40);
    KMU_TRY(launch(ctx, "k_read_anchors", k_read_anchors, dim3(grid), dim3(64), 0, a));
    KMU_TRY(bring_output(ctx, hashes_out, a.hashes_out, rows * m, p->mem));
    KMU_TRY(bring_output(ctx, counts_out, a.counts_out, rows * m, p->mem));
    KMU_TRY(bring_output(ctx, n_out, a.n_out, rows, p->mem));
    return finish_checked(ctx, p->mem, a.err);
}

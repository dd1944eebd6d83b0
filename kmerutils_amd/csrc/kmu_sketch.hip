// kmu_sketch.hip -- the C entry points of the sketch unit (kmu_sketch / kmu_sketch_hashed / kmu_sketch_partial /
// kmu_sketch_hashed_partial / kmu_sketch_merge_partials / kmu_kmer_hashes_compact), the all-sequences path and the steps the
// unit's files share: parameter checks, compact hashing, the per-sequence dispatch (kmu_sketch_host.hpp).  The ProbMinHash3a /
// bottom-k routes are in kmu_sketch_pmh.hip, kmu_sketch_count in kmu_sketch_pipe.hip, kmu_sketch_groups in kmu_sketch_groups.hip.
// Reference: SeqSketcherT::sketch_compressedkmer / sketch_compressedkmer_seqs (src/sketching/setsketchert.rs:54-80,
// seqsketchjaccard.rs:211-319), datasketcher's loop (src/bin/datasketcher.rs:222-226).  The kernels are in kmu_pmh_*.hip (one file per route) and kmu_sketch_aux.hip.
#include <algorithm>

#include "kmu_sketch_host.hpp"
#include "kmu_sketch_kernels.h"

using namespace kmu;

static int sketch_params_check(kmu_ctx *ctx, const kmu_sketch_params *p) {
    if (p->sketch_size < (p->algo == KMU_ALGO_BOTTOMK ? 1 : 2) || p->sketch_size > 65536)
        return fail(ctx, KMU_E_BAD_ARG, "sketch_size %d out of range", p->sketch_size);
    int w = kmer_val_bytes(p->kmer_type);
    switch (p->algo) {
    case KMU_ALGO_PROB3A:
        if (p->sig_type != (w == 4 ? KMU_SIG_U32 : KMU_SIG_U64))
            return fail(ctx, KMU_E_BAD_ARG, "ProbMinHash3a signature type is Kmer::Val (setsketchert.rs:107)");
        if (p->hasher != KMU_HASHER_NOHASH)
            return fail(ctx, KMU_E_BAD_ARG, "ProbMinHash3a is always built with NoHashHasher (seqsketchjaccard.rs:235)");
        break;
    case KMU_ALGO_SUPER:
        if (p->sig_type != KMU_SIG_F32 && p->sig_type != KMU_SIG_F64) return fail(ctx, KMU_E_BAD_ARG, "SuperMinHash signature is f32/f64");
        break;
    case KMU_ALGO_OPTDENS:
    case KMU_ALGO_REVOPTDENS:
        if (p->sig_type != KMU_SIG_F32 && p->sig_type != KMU_SIG_F64) return fail(ctx, KMU_E_BAD_ARG, "OptDens / RevOptDens signature is f32/f64");
        break;
    case KMU_ALGO_HLL:
        if (p->sig_type != KMU_SIG_U16 && p->sig_type != KMU_SIG_U32 && p->sig_type != KMU_SIG_U64)
            return fail(ctx, KMU_E_BAD_ARG, "SetSketch registers are u16 / u32 / u64");
        if (p->sig_type == KMU_SIG_U16 && ctx->hll.q + 1 > 65535u) return fail(ctx, KMU_E_BAD_ARG, "q + 1 does not fit u16 registers");
        break;
    case KMU_ALGO_SUPER2:
        if (p->sig_type != KMU_SIG_U32 && p->sig_type != KMU_SIG_U64) return fail(ctx, KMU_E_BAD_ARG, "SuperMinHash2 signature is u32/u64");
        break;
    case KMU_ALGO_BOTTOMK:
        if (p->sig_type != KMU_SIG_U64) return fail(ctx, KMU_E_BAD_ARG, "bottom-k rows are u64 hashes");
        break;
    default: return fail(ctx, KMU_E_BAD_ARG, "unknown algo %d", p->algo);
    }
    if (p->block_size < 0) return fail(ctx, KMU_E_BAD_ARG, "negative block_size");
    if (p->block_size > 0 && (p->algo != KMU_ALGO_PROB3A || p->mode != KMU_MODE_PER_SEQ))
        return fail(ctx, KMU_E_UNSUPPORTED, "block sketching is ProbMinHash3a per sequence (seqblocksketch.rs:97)");
    return KMU_OK;
}

// ProbMinHash3 (sketch_probminhash3, seqsketchjaccard.rs:272-319) generates the same points per key as ProbMinHash3a
// and keeps the same per-slot minimum: it runs on the ProbMinHash3a kernel (whole sequences only, like upstream).
static int resolve_algo(kmu_ctx *ctx, const kmu_sketch_params *p_in, kmu_sketch_params *p) {
    *p = *p_in;
    if (p->algo == KMU_ALGO_PROB3) {
        if (p->block_size > 0) return fail(ctx, KMU_E_UNSUPPORTED, "block sketching is ProbMinHash3a per sequence (seqblocksketch.rs:97)");
        p->algo = KMU_ALGO_PROB3A;
    }
    return KMU_OK;
}

namespace kmu {

int sketch_seq_params(kmu_ctx *ctx, const kmu_sketch_params *p_in, int input_kind, kmu_sketch_params *p) {
    KMU_TRY(resolve_algo(ctx, p_in, p));
    KMU_TRY(check_kmer(ctx, p->kmer_type, p->kmer_size));
    KMU_TRY(sketch_params_check(ctx, p));
    return check_fhash_input(ctx, p->kmer_type, p->fhash, input_kind);
}

int sketch_params(kmu_ctx *ctx, const kmu_sketch_params *p_in, kmu_sketch_params *p) {
    KMU_TRY(sketch_seq_params(ctx, p_in, p_in->input_kind, p));
    if (p->mode == KMU_MODE_ALL_SEQS && p->algo == KMU_ALGO_BOTTOMK)
        return fail(ctx, KMU_E_UNSUPPORTED, "the reference has no bottom-k sketch over a list of sequences");
    return KMU_OK;
}

int launch_nk_scan(kmu_ctx *ctx, const DevSeqs &ds, int kmer_size, uint32_t *d_err, const uint64_t **koff) {
    uint64_t *q;
    KMU_TRY(dev_array(ctx, "all.koff", (size_t) ds.n_seq + 1, &q));
    KMU_TRY(launch(ctx, nullptr, k_nk_scan, dim3(1), dim3(1024), 0, ds.offsets, ds.n_seq, kmer_size, q, d_err));
    *koff = q;
    return KMU_OK;
}

int count_kmers(kmu_ctx *ctx, const DevSeqs &ds, int kmer_size, uint32_t *d_err, const uint64_t **koff, uint64_t *n_items) {
    KMU_TRY(launch_nk_scan(ctx, ds, kmer_size, d_err, koff));
    return read_back(ctx, {{n_items, *koff + ds.n_seq}});
}

int launch_hashes_compact(kmu_ctx *ctx, const DevSeqs &ds, const KmerCfg &cfg, const uint64_t *koff, uint64_t *d_out, uint32_t *d_err) {
    if (ds.n_seq) {
        // few sequences: every workgroup takes a share of every sequence instead of whole sequences
        const int spread = ds.n_seq < (uint32_t) ctx->num_cus * 4 ? 1 : 0;
        const int grid = spread ? ctx->num_cus * 8 : (int) std::min<uint32_t>(ds.n_seq, (uint32_t) ctx->num_cus * 8);
        KMU_TRY(launch(ctx, "k_seq_hashes_compact", k_seq_hashes_compact, dim3(grid), dim3(256), 0, ds.bases, ds.offsets, ds.packed_offsets, ds.n_seq,
                       ds.packed, ds.total_bytes, cfg, koff, d_out, d_err, spread));
    }
    return KMU_OK;
}

int hash_all_kmers(kmu_ctx *ctx, const DevSeqs &ds, const KmerCfg &cfg, uint32_t *d_err, const uint64_t **koff_out, const uint64_t **hashes,
                   uint64_t *n_items) {
    const uint64_t *koff;
    void *hk;
    KMU_TRY(count_kmers(ctx, ds, cfg.k, d_err, &koff, n_items));
    KMU_TRY(dev_buf(ctx, "all.hashes", *n_items * 8 + 64, &hk));
    KMU_TRY(launch_hashes_compact(ctx, ds, cfg, koff, (uint64_t *) hk, d_err));
    if (koff_out) *koff_out = koff;
    *hashes = (const uint64_t *) hk;
    return KMU_OK;
}

// One sketch over a device array of n pre-hashed values (u64, zero-extended Kmer::Val).
//  ProbMinHash3a: the keys are radix-partitioned by hash into leaves that fit the LDS multiset; every leaf is an
//  independent weighted set (disjoint keys), sketched into partial slot minima, merged per slot by (h, key).
//  SuperMinHash(2): items are independent; chunks are sketched separately and the slot values merged by min.
int sketch_all_hashed(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *d_vals, uint64_t n, void *d_sig, uint32_t *d_err) {
    const int m = p->sketch_size;
    if (p->algo == KMU_ALGO_PROB3A) {
        const int region_bits = (int) pmh_leaf_bits(n);
        const uint64_t *items, *bounds;
        KMU_TRY(partition_u64(ctx, d_vals, n, region_bits, &items, &bounds));
        const uint64_t n_leaves = 1ull << region_bits;
        uint64_t *pk, *ph;
        KMU_TRY(dev_array(ctx, "all.part_h", n_leaves * m, &ph));
        KMU_TRY(dev_array(ctx, "all.part_k", n_leaves * m, &pk));
        KMU_TRY(launch_pmh3a_leaves(ctx, p, items, bounds, (uint32_t) n_leaves, ph, pk, d_err));
        KMU_TRY(launch(ctx, "k_pmh_reduce", k_pmh_reduce, dim3(m), dim3(256), 0, ph, pk, n_leaves, m, (uint64_t) m, kmer_val_bytes(p->kmer_type),
                       d_sig, ctx->partial_out));
        return KMU_OK;
    }
    // SuperMinHash / SuperMinHash2
    const uint64_t n_chunks = super_chunk_count(n);
    std::vector<uint64_t> h_off(n_chunks + 1);
    for (uint64_t c = 0; c <= n_chunks; c++) h_off[c] = n * c / n_chunks;
    uint64_t *pr, *d_off;
    KMU_TRY(dev_array(ctx, "all.chunk_off", n_chunks + 1, &d_off));
    KMU_HIP(ctx, hipMemcpyAsync(d_off, h_off.data(), (n_chunks + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    KMU_HIP(ctx, hipStreamSynchronize(ctx->stream)); // h_off is a local
    KMU_TRY(dev_array(ctx, "all.part_rows", n_chunks * m, &pr));
    KMU_TRY(launch_super(ctx, p, hashed_seqs(d_vals, d_off, (uint32_t) n_chunks), nullptr, d_err, d_vals, 8, pr));
    return launch_super_reduce(ctx, p, pr, n_chunks, d_sig);
}

int sketch_per_seq_device(kmu_ctx *ctx, const kmu_sketch_params *p, const DevSeqs &ds, const uint64_t *d_block_rows, uint32_t *d_counts,
                          void *d_sig, uint32_t *d_err, const uint64_t *h_offsets) {
    switch (p->algo) {
    case KMU_ALGO_PROB3A: return sketch_pmh_per_seq(ctx, p, ds, d_block_rows, d_sig, d_err, h_offsets);
    case KMU_ALGO_SUPER:
    case KMU_ALGO_SUPER2: return launch_super(ctx, p, ds, d_sig, d_err, nullptr, 0, nullptr);
    case KMU_ALGO_OPTDENS:
    case KMU_ALGO_REVOPTDENS:
    case KMU_ALGO_HLL: return launch_dens(ctx, p, ds, d_sig, d_err, nullptr, 0);
    case KMU_ALGO_BOTTOMK: {
        PmhInputs in;
        in.d_counts = d_counts;
        return launch_pmh3a(ctx, p, ds, d_sig, d_err, in);
    }
    default: return fail(ctx, KMU_E_UNSUPPORTED, "no per-sequence kernel for algo %d", p->algo);
    }
}

} // namespace kmu

extern "C" int kmu_sketch(kmu_ctx *ctx, const kmu_sketch_params *p_in, const uint8_t *bases, const uint64_t *offsets,
                          const uint64_t *packed_offsets, uint32_t n_seq, const uint64_t *block_row_offsets,
                          void *sig_out, uint32_t *counts_out) {
    if (!ctx || !p_in || !sig_out) return KMU_E_BAD_ARG;
    kmu_sketch_params p_res;
    KMU_TRY(sketch_params(ctx, p_in, &p_res));
    const kmu_sketch_params *p = &p_res;
    if (p->block_size > 0 && !block_row_offsets) return fail(ctx, KMU_E_BAD_ARG, "block mode needs block_row_offsets");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, packed_offsets, n_seq, p->input_kind, p->mem, &ds));
    const size_t sigb = sig_elem_bytes(p->sig_type);
    const bool all = p->mode == KMU_MODE_ALL_SEQS, host_blocks = p->mem == KMU_MEM_HOST && p->block_size > 0;
    const uint64_t rows = all ? 1 : host_blocks ? block_row_offsets[n_seq] : n_seq; // (of a host call: what is copied down)
    const uint64_t *d_block_rows = nullptr;
    uint8_t *d_sig;
    uint32_t *d_counts;
    if (host_blocks || p->mem == KMU_MEM_DEVICE) KMU_TRY(stage_to_device(ctx, "in.blockrows", block_row_offsets, (size_t) n_seq + 1, p->mem, &d_block_rows));
    KMU_TRY(place_output(ctx, "out.sig", (uint8_t *) sig_out, rows * p->sketch_size * sigb + 64, p->mem, &d_sig));
    KMU_TRY(place_output(ctx, "out.counts", counts_out, rows * p->sketch_size + 16, p->mem, &d_counts));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    if (all && algo_is_dens(p->algo)) { // one set of bins for every sequence, filled in place (setsketchert.rs:429-463)
        KMU_TRY(launch_dens(ctx, p, ds, d_sig, d_err, nullptr, 0));
    } else if (all) {
        // sketch_compressedkmer_seqs (setsketchert.rs:160-202, :299-335): one multiset / one stream over every
        // sequence.  fhash values of all k-mers, compact; then the pre-hashed all-sequences path.
        const uint64_t *hk;
        uint64_t n_items = 0;
        KMU_TRY(hash_all_kmers(ctx, ds, KmerCfg{p->kmer_type, p->kmer_size, p->fhash}, d_err, nullptr, &hk, &n_items));
        KMU_TRY(sketch_all_hashed(ctx, p, hk, n_items, d_sig, d_err));
    } else if (n_seq) {
        KMU_TRY(sketch_per_seq_device(ctx, p, ds, d_block_rows, d_counts, d_sig, d_err, nullptr));
    }
    KMU_TRY(bring_output(ctx, (uint8_t *) sig_out, d_sig, rows * p->sketch_size * sigb, p->mem));
    if (!all) KMU_TRY(bring_output(ctx, counts_out, d_counts, rows * p->sketch_size, p->mem));
    return finish_checked(ctx, p->mem, d_err);
}

extern "C" int kmu_sketch_hashed(kmu_ctx *ctx, const kmu_sketch_params *p_in, const void *hashed, const uint64_t *offsets,
                                 uint32_t n_seq, void *sig_out, uint32_t *counts_out) {
    if (!ctx || !p_in || !sig_out || !offsets || (!hashed && n_seq)) return KMU_E_BAD_ARG;
    kmu_sketch_params p_res;
    KMU_TRY(resolve_algo(ctx, p_in, &p_res));
    const kmu_sketch_params *p = &p_res;
    KMU_TRY(sketch_params_check(ctx, p));
    if (p->block_size > 0) return fail(ctx, KMU_E_UNSUPPORTED, "block sketching needs the sequences (k-mer positions)");
    if (p->mode == KMU_MODE_ALL_SEQS && p->algo == KMU_ALGO_BOTTOMK)
        return fail(ctx, KMU_E_UNSUPPORTED, "the reference has no bottom-k sketch over a list of sequences");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const int w = kmer_val_bytes(p->kmer_type);
    const size_t sigb = sig_elem_bytes(p->sig_type);
    const int m = p->sketch_size;
    const uint64_t rows = p->mode == KMU_MODE_ALL_SEQS ? 1 : n_seq;
    const uint8_t *d_vals;
    const uint64_t *d_off;
    uint8_t *d_sig;
    uint32_t *d_counts;
    uint64_t n_items = 0, first_item = 0; // the values of the sequences are hashed[offsets[0] .. offsets[n_seq])
    if (p->mem == KMU_MEM_HOST) {
        n_items = offsets[n_seq];
        first_item = n_seq ? offsets[0] : 0;
    } else if (n_seq) KMU_TRY(read_back(ctx, {{&n_items, offsets + n_seq}, {&first_item, offsets}}));
    else KMU_TRY(read_back(ctx, {{&n_items, offsets + n_seq}}));
    KMU_TRY(stage_to_device(ctx, "in.bases", (const uint8_t *) hashed, n_items * w, p->mem, &d_vals, 64));
    KMU_TRY(stage_to_device(ctx, "in.offsets", offsets, (size_t) n_seq + 1, p->mem, &d_off));
    KMU_TRY(place_output(ctx, "out.sig", (uint8_t *) sig_out, rows * m * sigb + 64, p->mem, &d_sig));
    KMU_TRY(place_output(ctx, "out.counts", counts_out, rows * m + 16, p->mem, &d_counts));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    const DevSeqs ds = hashed_seqs(d_vals, d_off, n_seq);
    if (algo_is_dens(p->algo)) {
        KMU_TRY(launch_dens(ctx, p, ds, d_sig, d_err, d_vals, w));
    } else if (p->mode == KMU_MODE_ALL_SEQS) {
        n_items -= first_item;
        const uint64_t *v64 = (const uint64_t *) d_vals + first_item;
        if (w == 4) { // widen to u64 once (the all-sequences path partitions u64 keys)
            void *q;
            KMU_TRY(dev_buf(ctx, "all.hashes", n_items * 8 + 64, &q));
            KMU_TRY(launch(ctx, nullptr, k_widen_u32, dim3((unsigned) std::min<uint64_t>((n_items + 255) / 256 + 1, 65535)), dim3(256), 0,
                           (const uint32_t *) d_vals + first_item, n_items, (uint64_t *) q));
            v64 = (const uint64_t *) q;
        }
        KMU_TRY(sketch_all_hashed(ctx, p, v64, n_items, d_sig, d_err));
    } else if (n_seq) {
        if (p->algo == KMU_ALGO_SUPER || p->algo == KMU_ALGO_SUPER2) KMU_TRY(launch_super(ctx, p, ds, d_sig, d_err, d_vals, w, nullptr));
        else {
            PmhInputs in;
            in.d_counts = d_counts;
            in.hashed = d_vals;
            in.hashed_bytes = w;
            KMU_TRY(launch_pmh3a(ctx, p, ds, d_sig, d_err, in));
        }
    }
    KMU_TRY(bring_output(ctx, (uint8_t *) sig_out, d_sig, rows * m * sigb, p->mem));
    if (p->mode != KMU_MODE_ALL_SEQS) KMU_TRY(bring_output(ctx, counts_out, d_counts, rows * m, p->mem));
    return finish_checked(ctx, p->mem, d_err);
}

// ---- one signature for sequences held by several GPUs ------------------------------------------------------------------
// Every rank turns ITS share into per-slot minima (a "partial"), the ranks exchange these small arrays (all-gather) and each
// merges them.  SuperMinHash / SuperMinHash2 / OptDens / RevOptDens sketch k-mer occurrences independently, so a rank's share
// is simply its sequences.  ProbMinHash weighs a key by its multiplicity over ALL sequences: the shares must hold disjoint
// key sets (exchange the hashed k-mers by owner first, as counting does), then per-slot (h, key) minima merge exactly.
extern "C" uint32_t kmu_sketch_partial_words(const kmu_sketch_params *p) {
    if (!p || p->sketch_size < 1) return 0;
    const bool prob = p->algo == KMU_ALGO_PROB3A || p->algo == KMU_ALGO_PROB3;
    return (uint32_t) p->sketch_size * (prob ? 2u : 1u);
}

static int partial_begin(kmu_ctx *ctx, const kmu_sketch_params *p_in, kmu_sketch_params *p, uint64_t *partial_out, uint64_t **d_part) {
    if (!ctx || !p_in || !partial_out) return KMU_E_BAD_ARG;
    *p = *p_in;
    p->mode = KMU_MODE_ALL_SEQS;
    p->block_size = 0;
    if (p->algo == KMU_ALGO_BOTTOMK) return fail(ctx, KMU_E_UNSUPPORTED, "the reference has no bottom-k sketch over a list of sequences");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    return place_output(ctx, "out.partial", partial_out, (size_t) kmu_sketch_partial_words(p) + 8, p->mem, d_part);
}

static int partial_end(kmu_ctx *ctx, const kmu_sketch_params *p, int rc, uint64_t *partial_out, const uint64_t *d_part) {
    ctx->partial_out = nullptr;
    if (rc != KMU_OK) return rc;
    KMU_TRY(bring_output(ctx, partial_out, d_part, (size_t) kmu_sketch_partial_words(p), p->mem));
    if (p->mem == KMU_MEM_HOST) KMU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return KMU_OK;
}

extern "C" int kmu_sketch_partial(kmu_ctx *ctx, const kmu_sketch_params *p_in, const uint8_t *bases, const uint64_t *offsets,
                                  const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *partial_out) {
    kmu_sketch_params p;
    uint64_t *d_part = nullptr;
    KMU_TRY(partial_begin(ctx, p_in, &p, partial_out, &d_part));
    void *scratch_sig; // the signature slot of the inner call is not used
    KMU_TRY(dev_buf(ctx, "out.sig", (size_t) p.sketch_size * 8 + 64, &scratch_sig));
    std::vector<uint64_t> host_sig(p.mem == KMU_MEM_HOST ? (size_t) p.sketch_size : 0);
    ctx->partial_out = d_part;
    const int rc = kmu_sketch(ctx, &p, bases, offsets, packed_offsets, n_seq, nullptr,
                              p.mem == KMU_MEM_HOST ? (void *) host_sig.data() : scratch_sig, nullptr);
    return partial_end(ctx, &p, rc, partial_out, d_part);
}

extern "C" int kmu_sketch_hashed_partial(kmu_ctx *ctx, const kmu_sketch_params *p_in, const void *hashed, const uint64_t *offsets,
                                         uint32_t n_seq, uint64_t *partial_out) {
    kmu_sketch_params p;
    uint64_t *d_part = nullptr;
    KMU_TRY(partial_begin(ctx, p_in, &p, partial_out, &d_part));
    void *scratch_sig;
    KMU_TRY(dev_buf(ctx, "out.sig", (size_t) p.sketch_size * 8 + 64, &scratch_sig));
    std::vector<uint64_t> host_sig(p.mem == KMU_MEM_HOST ? (size_t) p.sketch_size : 0);
    ctx->partial_out = d_part;
    const int rc = kmu_sketch_hashed(ctx, &p, hashed, offsets, n_seq, p.mem == KMU_MEM_HOST ? (void *) host_sig.data() : scratch_sig,
                                     nullptr);
    return partial_end(ctx, &p, rc, partial_out, d_part);
}

extern "C" int kmu_sketch_merge_partials(kmu_ctx *ctx, const kmu_sketch_params *p_in, const uint64_t *partials, uint32_t n_parts,
                                         void *sig_out) {
    if (!ctx || !p_in || !partials || !sig_out || n_parts == 0) return KMU_E_BAD_ARG;
    kmu_sketch_params p_res;
    KMU_TRY(resolve_algo(ctx, p_in, &p_res));
    const kmu_sketch_params *p = &p_res;
    KMU_TRY(sketch_params_check(ctx, p));
    if (p->algo == KMU_ALGO_BOTTOMK) return fail(ctx, KMU_E_UNSUPPORTED, "no bottom-k sketch over a list of sequences");
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    const int m = p->sketch_size;
    const size_t sigb = sig_elem_bytes(p->sig_type);
    const uint64_t words = kmu_sketch_partial_words(p);
    const uint64_t *d_parts;
    uint8_t *d_sig;
    KMU_TRY(stage_to_device(ctx, "in.partials", partials, (size_t) n_parts * words, p->mem, &d_parts, 8));
    KMU_TRY(place_output(ctx, "out.sig", (uint8_t *) sig_out, (size_t) m * sigb + 64, p->mem, &d_sig));
    if (p->algo == KMU_ALGO_PROB3A) {
        KMU_TRY(launch(ctx, nullptr, k_pmh_reduce, dim3(m), dim3(256), 0, d_parts, d_parts + m, (uint64_t) n_parts, m, words,
                       kmer_val_bytes(p->kmer_type), d_sig, (uint64_t *) nullptr));
    } else if (algo_is_dens(p->algo)) {
        KMU_TRY(launch_dens_merge(ctx, p, d_parts, n_parts, d_sig));
    } else {
        KMU_TRY(launch_super_reduce(ctx, p, d_parts, n_parts, d_sig));
    }
    KMU_TRY(bring_output(ctx, (uint8_t *) sig_out, d_sig, (size_t) m * sigb, p->mem));
    return finish_call(ctx, p->mem);
}

// fhash of every k-mer of every sequence, one after the other (no gaps for the positions that start no k-mer): what a rank
// hands to the owner exchange of a distributed ProbMinHash sketch.  out == NULL: only the number of values in *n_out.
extern "C" int kmu_kmer_hashes_compact(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets,
                                       const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *out, uint64_t cap, uint64_t *n_out) {
    if (!ctx || !p || !n_out) return KMU_E_BAD_ARG;
    KMU_TRY(check_hash_params(ctx, p));
    KMU_HIP(ctx, hipSetDevice(ctx->device));
    *n_out = 0;
    if (n_seq == 0) return KMU_OK;
    DevSeqs ds;
    KMU_TRY(stage_sequences(ctx, bases, offsets, packed_offsets, n_seq, p->input_kind, p->mem, &ds));
    uint32_t *d_err;
    KMU_TRY(get_err_word(ctx, &d_err));
    const uint64_t *koff;
    uint64_t n_items = 0;
    KMU_TRY(count_kmers(ctx, ds, p->kmer_size, d_err, &koff, &n_items));
    *n_out = n_items;
    if (!out) return KMU_OK;
    if (cap < n_items) return fail(ctx, KMU_E_BAD_ARG, "output too small: %llu values", (unsigned long long) n_items);
    uint64_t *d_out;
    KMU_TRY(place_output(ctx, "all.hashes", out, n_items + 8, p->mem, &d_out));
    KMU_TRY(launch_hashes_compact(ctx, ds, KmerCfg{p->kmer_type, p->kmer_size, p->fhash}, koff, d_out, d_err));
    KMU_TRY(bring_output(ctx, out, d_out, n_items, p->mem));
    return finish_checked(ctx, p->mem, d_err);
}

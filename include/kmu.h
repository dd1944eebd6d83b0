/*
 * kmu.h -- C-ABI boundary of the MI355X (gfx950) k-mer generation + counting + sketching hot path.
 *
 * This is the drop-in boundary for the hot path of jean-pierreBoth/kmerutils (a Rust crate with no FFI of its
 * own): every entry point below replaces a *Rust* interface of the reference, cited as `file:line` relative
 * to the reference tree.  A Rust closure cannot cross an FFI, so the `fhash` closures the reference actually
 * uses are enumerated in `kmu_fhash`.  INTEGRATION.md shows the `extern "C"` block and the
 * `impl SeqSketcherT<Kmer> for ...` shim a maintainer would add on the Rust side.
 *
 * Conventions
 *  - plain C scalars / pointers / sizes only; no torch, no C++ types.
 *  - every call returns 0 (KMU_OK) or a negative kmu_status; kmu_last_error() gives the text.
 *  - the caller owns every input and output buffer.  `mem` says where they live:
 *      KMU_MEM_HOST   : host pointers; the library stages H2D / D2H itself (synchronous call).
 *      KMU_MEM_DEVICE : HIP device pointers (e.g. a torch tensor's data_ptr()); kernels are enqueued on the
 *                       context's stream and the call returns after the stream has been synchronised unless
 *                       the context was created with `async_device = 1`.  Such calls cannot report what their kernels
 *                       find (a non-ACGT byte, an empty sequence, a full table): the device error word is sticky, and
 *                       the bits of every call since the last synchronising call come back from the next one --
 *                       kmu_synchronize at the latest.
 *  - sequences are handed over as one concatenated byte array + (n_seq+1) uint64 offsets:
 *      KMU_INPUT_ASCII  : bases[offsets[i] .. offsets[i+1]) are the ASCII letters of sequence i
 *      KMU_INPUT_PACKED2: offsets are in *bases*; sequence i starts at byte `packed_byte_offsets[i]`
 *                         and is packed exactly as reference `Sequence::new(raw,2)`
 *                         (src/base/sequence.rs:48-73: 4 bases / byte, first base in bits 7..6).
 *    offsets[0] need not be 0: `offsets + first` with n_seq = last - first names the reads [first, last) of a larger
 *    array without copying anything (the base pointer stays the array's).
 *  - a kmu_ctx is used from one thread at a time; distinct contexts may run concurrently.
 */
#ifndef KMU_H
#define KMU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KMU_VERSION_MAJOR 0
#define KMU_VERSION_MINOR 1

typedef struct kmu_ctx kmu_ctx;
typedef struct kmu_counter kmu_counter;

typedef enum kmu_status {
    KMU_OK = 0,
    KMU_E_BAD_K = -1,        /* reference: panic in KmerSeqIterator::new, src/base/kmergenerator.rs:48-53 */
    KMU_E_BAD_ALPHABET = -2,
    KMU_E_EMPTY_SEQ = -3,    /* reference: ilog2(0) panic, src/sketching/nbkmerguess.rs:8 */
    KMU_E_NON_ACGT = -4,     /* reference: Alphabet2b::encode panics, src/base/alphabet.rs:125 */
    KMU_E_OOM = -5,
    KMU_E_HIP = -6,
    KMU_E_BAD_ARG = -7,
    KMU_E_TABLE_FULL = -8,
    KMU_E_UNSUPPORTED = -9,
    KMU_E_NO_DEVICE = -10,
    KMU_E_RCCL = -11         /* RCCL (or the host's transport) reported an error; text in kmu_last_error */
} kmu_status;

typedef enum kmu_mem { KMU_MEM_HOST = 0, KMU_MEM_DEVICE = 1 } kmu_mem;
typedef enum kmu_input_kind { KMU_INPUT_ASCII = 0, KMU_INPUT_PACKED2 = 1 } kmu_input_kind;

/* k-mer value types of the reference (src/base/kmer32bit.rs:22, kmer16b32bit.rs:21, kmer64bit.rs:24,
 * src/aautils/kmeraa.rs:146,280).  The type fixes Kmer::Val (u32 / u64) and the bit layout of `.0`. */
typedef enum kmu_kmer_type {
    KMU_KMER32BIT = 0,    /* k <= 14, u32, k stored in bits 31..28            */
    KMU_KMER16B32BIT = 1, /* k == 16, u32                                     */
    KMU_KMER64BIT = 2,    /* k <= 31, (u64, u8); k = 32 is broken upstream    */
    KMU_KMERAA32BIT = 3,  /* amino acids, 5 bits, k <= 6, u32                 */
    KMU_KMERAA64BIT = 4   /* amino acids, 5 bits, k <= 12, u64                */
} kmu_kmer_type;

/* The closures `fhash: Fn(&Kmer) -> Kmer::Val` that reference callers really pass. */
typedef enum kmu_fhash {
    KMU_FHASH_IDENTITY_RAW = 0,   /* kmer.0                      src/sketching/seqsketchjaccard.rs:775,883 */
    KMU_FHASH_VALUE_MASKED = 1,   /* get_compressed_value() & mask   src/sketching/setsketchert.rs:1098-1104,
                                                                     src/aautils/setsketchert.rs:1235-1241 */
    KMU_FHASH_CANON_RAW = 2,      /* min(kmer, revcomp).0        src/base/kmercount.rs:313 */
    KMU_FHASH_CANON_INVHASH = 3,  /* intNN_hash(min(kmer,revcomp).0)  src/bin/datasketcher.rs:222-226,
                                                                      src/sketching/seqsketchjaccard.rs:931-935 */
    KMU_FHASH_INVHASH_RAW = 4,    /* intNN_hash(kmer.0)          src/sketching/seqminhash.rs:38,49 */
    KMU_FHASH_CANON_VALUE = 5,    /* min(kmer, revcomp).get_compressed_value()  src/base/kmercount.rs:313-316 */
    KMU_FHASH_CANON_NTHASH = 6,   /* canonical ntHash, 2-bit seed table  src/base/kmer.rs:76-95 (any k) */
    KMU_FHASH_CANON_NTHASH_8B = 7 /* canonical ntHash with the reference's ASCII table, bug-compatible:
                                     'G' and 'T' map to seed 0   src/base/nthash.rs:48-57,214-228 */
} kmu_fhash;

typedef enum kmu_algo {
    KMU_ALGO_PROB3A = 0, /* ProbMinHash3a  (probminhash crate), src/sketching/seqsketchjaccard.rs:211-260 */
    KMU_ALGO_SUPER = 1,  /* SuperMinHash   (probminhash crate), src/sketching/setsketchert.rs:255-297 */
    KMU_ALGO_SUPER2 = 2, /* SuperMinHash2  (integer sketch),   src/sketching/setsketchert.rs:963-1004.
                          * PROVISIONAL: the crate's fixed-point arithmetic is not in the reference tree; reference parity
                          * cannot be established in this build environment */
    KMU_ALGO_BOTTOMK = 3, /* MinHashCount / MinInvHashCountKmer, src/sketching/minhash.rs:62-99,219-265 */
    KMU_ALGO_PROB3 = 4,   /* ProbMinHash3 (SeqSketcher::sketch_probminhash3, seqsketchjaccard.rs:272-319): the same point
                           * process as ProbMinHash3a handled key by key; the signature is the same per-slot arg-min */
    /* PROVISIONAL (5, 6, 7): scheme from the cited papers, inner hash / variant choices of the `probminhash` crate
     * unknown here; reference parity impossible in this build environment */
    KMU_ALGO_OPTDENS = 5, /* OptDensHashSketch: one-permutation hashing + optimal densification (Shrivastava 2017),
                           * src/sketching/setsketchert.rs:343-463, src/aautils/setsketchert.rs:482-612; sig F32 / F64 */
    KMU_ALGO_REVOPTDENS = 6, /* RevOptDensHashSketch: the same with reverse densification (Mai et al. 2019), meant for
                           * sketches larger than the sequences, setsketchert.rs:474-599, aautils/setsketchert.rs:616-746 */
    KMU_ALGO_HLL = 7      /* HyperLogLogSketch: SetSketch registers (Ertl 2021), setsketchert.rs:640-896,
                           * aautils/setsketchert.rs:780-1011; sig U16 / U32 / U64; parameters: kmu_set_hll_params */
} kmu_algo;

typedef enum kmu_sig_type { KMU_SIG_U32 = 0, KMU_SIG_U64 = 1, KMU_SIG_F32 = 2, KMU_SIG_F64 = 3, KMU_SIG_U16 = 4 /* HLL only */ } kmu_sig_type;

/* std::hash::Hasher used to seed the per-element RNG */
typedef enum kmu_hasher {
    KMU_HASHER_NOHASH = 0, /* src/nohasher.rs:11-49: finish() = byte-swapped key on little-endian hosts */
    KMU_HASHER_FNV1A = 1,  /* fnv::FnvHasher, src/sketching/seqsketchjaccard.rs:346-349 */
    KMU_HASHER_INT64HASH = 2 /* BOTTOMK only: int64_hash(value as u64), MinInvHashCountKmer minhash.rs:223-233 */
} kmu_hasher;

typedef enum kmu_sketch_mode {
    KMU_MODE_PER_SEQ = 0, /* sketch_compressedkmer: one signature per sequence      setsketchert.rs:121-157 */
    KMU_MODE_ALL_SEQS = 1 /* sketch_compressedkmer_seqs: one signature for all       setsketchert.rs:160-202 */
} kmu_sketch_mode;

/* flags */
#define KMU_FLAG_RAND08 0x1u /* index draws as rand 0.8 `Uniform<usize>` (64-bit widening multiply) instead of
                                rand 0.9 (32-bit when the range fits u32); see DESIGN.md "unpinned" */

typedef struct kmu_device_cfg {
    int32_t device_id;     /* HIP device ordinal */
    int32_t async_device;  /* 1: KMU_MEM_DEVICE calls return without synchronising the stream */
    void *stream;          /* hipStream_t to enqueue on, or NULL to let the library create one */
    uint64_t workspace_bytes; /* 0 = grow on demand */
} kmu_device_cfg;

typedef struct kmu_sketch_params {
    int32_t algo;        /* kmu_algo */
    int32_t kmer_type;   /* kmu_kmer_type */
    int32_t kmer_size;
    int32_t sketch_size; /* m */
    int32_t sig_type;    /* kmu_sig_type; PROB3A/BOTTOMK: must match Kmer::Val width; SUPER / OPTDENS / REVOPTDENS: F32/F64 */
    int32_t hasher;      /* kmu_hasher */
    int32_t fhash;       /* kmu_fhash */
    int32_t block_size;  /* 0 = whole sequence; >0 = BlockSeqSketcher (src/sketching/seqblocksketch.rs:97-149) */
    int32_t mode;        /* kmu_sketch_mode */
    int32_t input_kind;  /* kmu_input_kind */
    int32_t mem;         /* kmu_mem */
    uint32_t flags;
} kmu_sketch_params;

typedef struct kmu_hash_params {
    int32_t kmer_type;
    int32_t kmer_size;
    int32_t fhash;
    int32_t input_kind;
    int32_t mem;
    uint32_t flags;
} kmu_hash_params;

typedef struct kmu_count_params {
    int32_t kmer_type;     /* DNA types only */
    int32_t kmer_size;
    int32_t counter_bits;  /* 8 or 16 (reference default 8: saturates at 255, src/base/kmercount.rs:1615) */
    int32_t flags;         /* 0, or KMU_COUNT_DISTRIBUTED [| KMU_COUNT_OWNER_HASH] (see "multi-GPU" below), KMU_COUNT_HINT_OCCURRENCES */
    uint64_t capacity_hint; /* expected number of distinct canonical k-mers (KMU_COUNT_HINT_OCCURRENCES: of k-mer occurrences) */
} kmu_count_params;

/* ---- context ------------------------------------------------------------------------------------- */
const char *kmu_version(void);
int kmu_device_count(void);
int kmu_create(const kmu_device_cfg *cfg, kmu_ctx **out);
void kmu_destroy(kmu_ctx *ctx);
const char *kmu_last_error(const kmu_ctx *ctx); /* ctx may be NULL: last error of a failed kmu_create */
int kmu_synchronize(kmu_ctx *ctx);
void *kmu_stream(kmu_ctx *ctx); /* the hipStream_t kernels are enqueued on */

/* Device buffers for callers that have no HIP binding of their own (a Rust or C host): allocate on the context's device,
 * copy in / out on the context's stream (both copies return when the data has arrived), then hand the pointers to the
 * KMU_MEM_DEVICE form of every entry point -- reads uploaded once can be ingested, sketched and counted without
 * crossing PCIe again.  kmu_dev_free waits for the context's stream first. */
int kmu_dev_alloc(kmu_ctx *ctx, uint64_t bytes, void **out);
int kmu_dev_free(kmu_ctx *ctx, void *p);
/* pinned host memory (hipHostMalloc): uploads from it and downloads into it are real DMA transfers that overlap kernels */
int kmu_host_alloc(kmu_ctx *ctx, uint64_t bytes, void **out);
int kmu_host_free(kmu_ctx *ctx, void *p);
int kmu_copy_to_device(kmu_ctx *ctx, void *dst_device, const void *src_host, uint64_t bytes);
int kmu_copy_to_host(kmu_ctx *ctx, void *dst_host, const void *src_device, uint64_t bytes);

/* SetSketchParams of the following KMU_ALGO_HLL calls on this context (probminhash::setsketcher::SetSketchParams, passed to
 * HyperLogLogSketch::new, setsketchert.rs:660-672): register base b > 1, rate a > 0, register limit q (values 0 .. q + 1).
 * m is the call's sketch_size.  Defaults: b = 1.001, a = 20, q = 65534. */
typedef struct kmu_hll_params {
    double b;
    double a;
    uint32_t q;
    uint32_t reserved;
} kmu_hll_params;
int kmu_set_hll_params(kmu_ctx *ctx, const kmu_hll_params *hp);

/* per-kernel device timing with hipEvents on the context stream (bench.py roofline object) */
int kmu_profile_enable(kmu_ctx *ctx, int on);
int kmu_profile_reset(kmu_ctx *ctx);
/* returns number of kernels known; fills up to `cap` entries */
typedef struct kmu_kernel_stat {
    char name[48];
    uint64_t launches;
    double total_ms;
} kmu_kernel_stat;
int kmu_profile_get(kmu_ctx *ctx, kmu_kernel_stat *stats, int cap);

/* ---- L0: alphabet + Sequence::new(raw, 2)  (src/base/alphabet.rs:119-127,162-168; sequence.rs:25-106) ---- */
/* number of bytes b with !is_acgt(b) per sequence (alphabet.rs:28-31); counts_out[n_seq] */
int kmu_count_non_acgt(kmu_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                       uint64_t *counts_out);
/* pack every sequence as Sequence::new(raw,2).  packed_offsets_out[n_seq+1] (bytes) is written first;
 * packed_out must hold sum(ceil(L_i/4)) bytes.  Returns KMU_E_NON_ACGT if any byte is not in ACGTacgt. */
int kmu_pack2b(kmu_ctx *ctx, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
               uint8_t *packed_out, uint64_t *packed_offsets_out);

/* ---- L1/L2: k-mer generation + canonicalise + hash, one value per k-mer start position -------------
 * KmerSeqIterator::next (src/base/kmergenerator.rs:75-106) followed by the fhash closure.
 * out[offsets[i] + p] (uint64, zero-extended for u32 types) for p in [0, L_i-k+1); other entries (the last k-1 positions
 * of a sequence) untouched in KMU_MEM_DEVICE arrays, zero in KMU_MEM_HOST arrays (the array comes back whole).
 * For KMU_INPUT_PACKED2 `packed_offsets` gives the byte offset of every sequence (may be NULL for ASCII). */
int kmu_kmer_hashes(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets,
                    const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *out);

/* KmerGenerationPattern::generate_kmer_pattern_in_range (src/base/kmergenerator.rs:126; impls :271-303,368-408,491-526;
 * amino acids src/aautils/kmeraa.rs:780-812,870-899): the k-mers that lie inside bases [range_begin[i], range_end[i]) of
 * sequence i -- KmerSeqIterator::set_range (kmergenerator.rs:66-68) on IterSequence::set_range (src/base/sequence.rs:562-585).
 * out[offsets[i] + p] for p in [range_begin[i], range_end[i] - k]; other entries untouched.  A range with end <= begin or
 * end > L_i is the reference's `Err(())` (unwrapped by its callers: a panic): KMU_E_BAD_ARG.  (The reference's debug build
 * also underflows for end < 4, sequence.rs:574; a release build wraps back to the intended byte: ends 1..3 are served.) */
int kmu_kmer_hashes_range(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets,
                          const uint64_t *packed_offsets, uint32_t n_seq, const uint64_t *range_begin,
                          const uint64_t *range_end, uint64_t *out);

/* KmerGenerationPattern::generate_kmer_distribution / KmerGenerator::generate_weighted_kmer (kmergenerator.rs:130,176; impls
 * :245-269,339-366,447-489; amino acids kmeraa.rs:752-778,845-868): the DISTINCT values fhash(kmer) of every sequence with
 * their multiplicities (u32 like the reference's FnvHashMap<T, u32>).  The pairs of sequence i are
 * kmers_out / mult_out [dist_offsets_out[i] .. dist_offsets_out[i + 1]), in no particular order (a hash map upstream).
 * Call with kmers_out == NULL for the sizes: *n_out = number of pairs, dist_offsets_out (n_seq + 1 entries, may be NULL).
 * KMU_FHASH_IDENTITY_RAW gives the k-mers themselves (`.0`), what the reference's map is keyed by. */
int kmu_kmer_distribution(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets,
                          const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *kmers_out, uint32_t *mult_out,
                          uint64_t cap, uint64_t *dist_offsets_out, uint64_t *n_out);

/* ntHash per k-mer position (src/base/nthash.rs; NtHash for 2-bit k-mers src/base/kmer.rs:45-145).
 *   table KMU_NTHASH_TABLE_2B: seeds of BASE_MAPPING_2B (nthash.rs:28-30) -- Kmer32bit / Kmer16b32bit::nthash_init,
 *                              nthash_canonical_init (kmer.rs:48-95); ASCII or packed input
 *         KMU_NTHASH_TABLE_8B: the reference's ASCII table BASE_MAPPING_8B bug for bug ('G' and 'T' hit zero entries,
 *                              nthash.rs:48-57) -- nthash_init_8b :153-161, nthash_rcomp_init_8b :182-189,
 *                              nthash_canonical_init_8b :214-228; upper-case ASCII input only
 *   mode  KMU_NTHASH_CANONICAL: min(forward, rcomp) and its strand (0 forward, 1 reverse; forward on ties, :223-227)
 *         KMU_NTHASH_FORWARD / KMU_NTHASH_RCOMP: one strand only (strand byte 0 / 1)
 *   n_hashes > 1: from_one_hash_val_to_mult_hash (:63-72) -- nthash_mult_canonical_init_8b :255-269, kmer.rs:123-131.
 * hashes_out[(offsets[i] + p) * n_hashes + j], strand_out[offsets[i] + p] (may be NULL) for p in [0, L_i - k + 1).
 * The value at every position is the *_init value of the k-mer starting there = what a correct roll reaches (the property
 * the reference tests, nthash.rs:333,379).  Not reproduced: the state resets that make the reference's own
 * nthash_mult_canonical_cycle_8b (:279-280) and the 2-bit nthash_canonical_cycle (kmer.rs:98-99) differ from their init forms.
 * 1 <= kmer_size <= 32. */
typedef enum kmu_nthash_mode { KMU_NTHASH_CANONICAL = 0, KMU_NTHASH_FORWARD = 1, KMU_NTHASH_RCOMP = 2 } kmu_nthash_mode;
typedef enum kmu_nthash_table { KMU_NTHASH_TABLE_2B = 0, KMU_NTHASH_TABLE_8B = 1 } kmu_nthash_table;
typedef struct kmu_nthash_params {
    int32_t kmer_size;
    int32_t table;      /* kmu_nthash_table */
    int32_t mode;       /* kmu_nthash_mode */
    int32_t n_hashes;   /* >= 1 */
    int32_t input_kind; /* kmu_input_kind */
    int32_t mem;        /* kmu_mem */
} kmu_nthash_params;
int kmu_nthash(kmu_ctx *ctx, const kmu_nthash_params *p, const uint8_t *bases, const uint64_t *offsets,
               const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *hashes_out, uint8_t *strand_out);

/* The same values without the gaps: fhash of every k-mer of sequence 0, then of sequence 1, ... (uint64, zero-extended).
 * Call with out == NULL for the number of values in *n_out.  (What a rank feeds to the owner exchange of a distributed
 * ProbMinHash sketch, see kmu_sketch_hashed_partial.) */
int kmu_kmer_hashes_compact(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets,
                            const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *out, uint64_t cap, uint64_t *n_out);

/* ---- L3 sketching: SeqSketcherT::sketch_compressedkmer{,_seqs}  (src/sketching/setsketchert.rs:54-80),
 * SeqSketcher::sketch_probminhash3a / sketch_superminhash (src/sketching/seqsketchjaccard.rs:211,328),
 * BlockSeqSketcher::blocksketch_sequences (src/sketching/seqblocksketch.rs:152-167),
 * SeqSketcherAAT (src/aautils/setsketchert.rs:42-72) ------------------------------------------------
 * sig_out: PER_SEQ, block_size == 0 : n_seq rows of sketch_size signatures, row i <-> sequence i
 *          PER_SEQ, block_size  > 0 : rows block_row_offsets[i] .. block_row_offsets[i+1], one row per block
 *                                     (block_row_offsets from kmu_block_layout; may be NULL if block_size==0)
 *          ALL_SEQS                 : 1 row
 * BOTTOMK: sig_out rows are sketch_size uint64 hashes ascending, padded with UINT64_MAX; counts_out (may be
 *          NULL) gets sketch_size uint32 multiplicities per row.
 * sketch_size: 2 .. 65536 (BOTTOMK: 1 .. 65536), KMU_E_BAD_ARG outside.  SUPER and SUPER2: 2 .. 8872; 8873 and above are
 *          KMU_E_UNSUPPORTED, returned before any kernel is launched, in every mode and for kmu_sketch_hashed, kmu_sketch_groups
 *          and kmu_sketch_partial alike (the context stays usable).  Why: a workgroup keeps the sketch in the 160 KiB of LDS of
 *          a CU -- 16 sketch_size + 4128 bytes of slot minima, index bounds and staged k-mers, and per k-mer in flight a
 *          permutation of sketch_size entries, of one byte up to sketch_size 256 and two above.  Above 1109 fewer than 64 k-mers
 *          are in flight (2500: 23, 8872: one); at 8873, 18 sketch_size + 4128 bytes exceed the 160 KiB. */
int kmu_sketch(kmu_ctx *ctx, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets,
               const uint64_t *packed_offsets, uint32_t n_seq, const uint64_t *block_row_offsets, void *sig_out,
               uint32_t *counts_out);
/* One signature per GROUP of consecutive sequences: row g = sketch_compressedkmer_seqs over the sequences
 * [group_offsets[g], group_offsets[g+1]) -- what gsearch does per genome / proteome file (setsketchert.rs:160-202, 299-335,
 * 1007-1045) --, bit for bit the row kmu_sketch gives in mode ALL_SEQS for those sequences alone.
 * group_offsets: n_groups + 1 sequence indices, group_offsets[0] == 0, non-decreasing, group_offsets[n_groups] == n_seq
 * (KMU_E_BAD_ARG otherwise, before any kernel reads through them); it lives where `offsets` lives (p->mem).  An empty group is
 * allowed and gets the ALL_SEQS row of n_seq = 0.  sig_out: n_groups rows of sketch_size signatures.  n_groups == 0: KMU_OK,
 * nothing is written.  p->mode is ignored; block_size > 0 and KMU_ALGO_BOTTOMK are KMU_E_UNSUPPORTED; what the kernels find
 * (KMU_E_NON_ACGT, KMU_E_EMPTY_SEQ, ...) is reported as kmu_sketch reports it, with the same sticky rules in async_device contexts.
 * Routes:  every algorithm takes one batched pass over all groups -- the kernel launches and the host synchronisations (at most
 *          one small device-to-host copy) of a call do not depend on n_groups.
 *          PROB3A, PROB3, SUPER, SUPER2: the k-mer hashes of all sequences, cut into leaves / chunks per group, one sketch
 *          kernel over all of them, one reduction per group.
 *          OPTDENS, REVOPTDENS, HLL (context's kmu_set_hll_params): no hash array; one persistent kernel walks tiles of equally
 *          many bases of the concatenated sequences into one row of bins / registers per group (8 * sketch_size bytes of
 *          workspace per group), one kernel densifies and stores the rows.  Neither the launches nor the load of the device
 *          depend on how the bases are cut into sequences and groups (sequences above 2^20 k-mers included). */
int kmu_sketch_groups(kmu_ctx *ctx, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets,
                      const uint64_t *packed_offsets, uint32_t n_seq, const uint64_t *group_offsets, uint32_t n_groups,
                      void *sig_out);
/* nb_blocks_i = ceil(L_i / block_size) (seqblocksketch.rs:108-112); block_row_offsets_out[n_seq+1], host memory,
 * offsets in host memory */
int kmu_block_layout(const uint64_t *offsets, uint32_t n_seq, uint32_t block_size, uint64_t *block_row_offsets_out);

/* ---- read anchors: bottom-k sketches of overlapping windows of every read -----------------------------------------
 * ReadAnchors / AnchorsGeneratorParameters (src/anchor.rs:228-329): a read of L bases is cut into slices of `window` bases
 * that overlap by `overlap` bases (stride = window - overlap; window > 0 and window > overlap, anchor.rs:295-296, else
 * KMU_E_BAD_ARG).  Slice s starts at beg = s * stride for every beg < L (anchor.rs:307-318): ceil(L / stride) slices, none for
 * L = 0 (not an error).  Its range is [beg, end) with end = min(beg + window, L - 1) (anchor.rs:242: the reference's
 * `seq.size() - 1` is kept, the last base of a read lies in no anchor), its k-mers those lying wholly inside the range
 * (IterSequence::set_range, sequence.rs:562-585): max(0, end - beg - k + 1) of them.
 * The row of a slice is bit for bit the row (and the counts) kmu_sketch gives for the bases [beg, end) handed over as a
 * sequence of their own with KMU_ALGO_BOTTOMK: the p->sketch_size (the reference's nbkmer) smallest hasher(fhash(kmer))
 * ascending, padded with UINT64_MAX; counts of padded entries are 0.  The reference's own anchors (MinInvHashCountKmer,
 * minhash.rs:204-289) are KMU_HASHER_INT64HASH + KMU_FHASH_VALUE_MASKED (u8 counts that wrap); every hasher / fhash pair
 * kmu_sketch accepts for BOTTOMK on DNA k-mers is accepted.  Column 0 of a non-empty row is the slice's index key
 * (get_minhash_key_for_redis, anchor.rs:149-158).
 * DEVIATION (the only one): a slice with end - beg < k -- beg == end included, which happens when L = 1 (mod stride) and
 * makes the reference panic (kmergenerator.rs:283-285) -- gets an empty row: all padding, n = 0.
 * Rows: anchor_row_offsets[i] .. anchor_row_offsets[i + 1] are the slices of read i, in order (kmu_anchor_layout).
 *   KMU_MEM_HOST: the library checks anchor_row_offsets against its own layout (KMU_E_BAD_ARG before any kernel runs).
 *   KMU_MEM_DEVICE: anchor_row_offsets lives where `offsets` lives and is trusted as kmu_sketch trusts block_row_offsets.
 * p: algo KMU_ALGO_BOTTOMK and block_size 0 (else KMU_E_BAD_ARG), 1 <= sketch_size <= KMU_ANCHOR_MAX_NBKMER (above:
 * KMU_E_UNSUPPORTED), input_kind KMU_INPUT_ASCII (KMU_INPUT_PACKED2: KMU_E_UNSUPPORTED), a DNA k-mer type (amino acids:
 * KMU_E_BAD_ALPHABET); p->mode is ignored.  A non-ACGT byte anywhere in a read is KMU_E_NON_ACGT, reported as kmu_sketch
 * reports it (sticky in async_device contexts).  More than 2^32 - 1 rows: KMU_E_UNSUPPORTED.  n_seq == 0 or no row at all:
 * KMU_OK, nothing is written.
 * One kernel launch per call whatever the number of reads and windows; a row reads its bases from the batch's base array
 * (nothing is copied per window) and selects in tiles of KMU_ANCHOR_TILE_KMERS k-mers, so no window size is refused. */
#define KMU_ANCHOR_MAX_NBKMER 256
#define KMU_ANCHOR_TILE_KMERS 768
/* rows per read: ceil(L_i / (window - overlap)); row_offsets_out[n_seq + 1]; host memory, like kmu_block_layout.  Plain host
 * C: no context, no device. */
int kmu_anchor_layout(const uint64_t *offsets, uint32_t n_seq, uint32_t window, uint32_t overlap, uint64_t *row_offsets_out);
int kmu_read_anchors(kmu_ctx *ctx, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                     uint32_t window, uint32_t overlap, const uint64_t *anchor_row_offsets,
                     uint64_t *hashes_out,   /* rows x p->sketch_size */
                     uint32_t *counts_out,   /* rows x p->sketch_size, may be NULL */
                     uint32_t *n_out);       /* rows: valid entries of each row, may be NULL */

/* The reads ONCE, both results: the per-sequence signatures of kmu_sketch and the k-mer counts of kmu_count_add_reads for
 * one batch of unpacked reads -- the reference's alternation "read a pack of sequences, sketch it" (src/bin/datasketcher.rs:
 * 243-260) and its counting pass (src/bin/parsefastq.rs:215-236) as one stream-ordered pipeline.
 *   p->mem == KMU_MEM_HOST   (bases, offsets, sig_out in host memory, best pinned: kmu_host_alloc): the bases cross PCIe
 *       once, in chunks of whole reads on an upload stream; the sketch kernels of chunk i run under the upload of chunk
 *       i + 1, the signature rows of chunk i go down on a download stream under the kernels that follow, and the count
 *       build runs on the resident reads under the last downloads.  Returns when everything is in host memory.
 *   p->mem == KMU_MEM_DEVICE: both results from the resident reads; a distributed counter's all-to-all is in flight
 *       while the reads are sketched.
 * counter may be NULL (signatures only).  Whole sequences, one signature per sequence (mode PER_SEQ, block_size 0), ASCII.
 * KMU_PIPE_CHUNK_MB sets the chunk size of the host form (default 512). */
int kmu_sketch_count(kmu_ctx *ctx, const kmu_sketch_params *p, kmu_counter *counter, const uint8_t *bases,
                     const uint64_t *offsets, uint32_t n_seq, void *sig_out);

/* fallback for arbitrary closures: the host evaluates fhash, the device does multiset + sketch only.
 * hashed[offsets[i] .. offsets[i+1]) are the hashed k-mers of sequence i (uint32 or uint64 per p->sig_type /
 * kmer_type width). */
int kmu_sketch_hashed(kmu_ctx *ctx, const kmu_sketch_params *p, const void *hashed, const uint64_t *offsets,
                      uint32_t n_seq, void *sig_out, uint32_t *counts_out);

/* One signature for sequences spread over several GPUs (sketch_compressedkmer_seqs across ranks, one process per GPU):
 * every rank turns its share into per-slot minima -- a "partial" of kmu_sketch_partial_words(p) uint64 words -- the ranks
 * exchange these small arrays (all-gather over RCCL) and every rank merges them into the signature.
 *   SuperMinHash / SuperMinHash2 / OptDens / RevOptDens treat k-mer occurrences independently: a rank's share is its reads.
 *   ProbMinHash weighs a key by its multiplicity over ALL sequences: the shares must be DISJOINT KEY SETS -- hash the k-mers
 *   (kmu_kmer_hashes), exchange the values by owner, and feed what a rank receives to kmu_sketch_hashed_partial.
 * `mode` and `block_size` of the parameters are ignored (one multiset over everything given); `mem` says where the partial
 * and the other buffers live.  A partial of no data at all merges as the neutral element. */
uint32_t kmu_sketch_partial_words(const kmu_sketch_params *p);
int kmu_sketch_partial(kmu_ctx *ctx, const kmu_sketch_params *p, const uint8_t *bases, const uint64_t *offsets,
                       const uint64_t *packed_offsets, uint32_t n_seq, uint64_t *partial_out);
int kmu_sketch_hashed_partial(kmu_ctx *ctx, const kmu_sketch_params *p, const void *hashed, const uint64_t *offsets, uint32_t n_seq,
                              uint64_t *partial_out);
/* partials: n_parts x kmu_sketch_partial_words(p) words; sig_out: sketch_size signatures */
int kmu_sketch_merge_partials(kmu_ctx *ctx, const kmu_sketch_params *p, const uint64_t *partials, uint32_t n_parts, void *sig_out);

/* ---- L3 counting: KmerCountT (src/base/kmercount.rs:48-59), KmerCounter::insert_kmer :241-267,
 * count_kmer_threaded_one_to_many :881-974, KmerCounterPool :424-565 --------------------------------- */
/* KMU_COUNT_HINT_OCCURRENCES (kmu_count_params.flags): capacity_hint counts the k-mer OCCURRENCES the caller is going to add (what
 * a caller knows: the bases of its reads), not distinct k-mers.  The table is then allocated by the first add and sized from the
 * duplication that add measures on a key sample of its batch (one extra pass over those reads, once per counter): occurrences /
 * ratio / 0.70 slots.  The reference's filters are sized the same blind way -- capacity 3e9 / n whatever the reads,
 * src/base/kmercount.rs:888-892 --; a table nine tenths empty costs nothing there, here every partitioned build writes the image.
 * Batches added later must fit the table the first one made (KMU_E_TABLE_FULL otherwise): give a distinct-k-mer hint where the
 * first batch is not representative.  Until that add kmu_count_table_info reports nslots = 0. */
#define KMU_COUNT_HINT_OCCURRENCES 0x4
int kmu_count_create(kmu_ctx *ctx, const kmu_count_params *p, kmu_counter **out);
void kmu_count_destroy(kmu_counter *c);
int kmu_count_reset(kmu_counter *c);
/* insert every canonical k-mer (min(kmer, revcomp), kmercount.rs:938) of every sequence */
int kmu_count_add_reads(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets,
                        const uint64_t *packed_offsets, uint32_t n_seq, int input_kind, int mem);
/* insert pre-computed canonical compressed values (KmerCountT::insert_kmer, one call per value) */
int kmu_count_add_kmers(kmu_counter *c, const uint64_t *canon_kmers, uint64_t n, int mem);
/* KmerCountT::get_count (kmercount.rs:270-277): 0 never seen, 1 singleton, else min(multiplicity, 2^bits-1) */
int kmu_count_query(kmu_counter *c, const uint64_t *canon_kmers, uint64_t n, int mem, uint32_t *counts_out);
int kmu_count_nb_distinct(kmu_counter *c, uint64_t *out); /* kmercount.rs:280-282 */
int kmu_count_nb_unique(kmu_counter *c, uint64_t *out);   /* kmercount.rs:285-287 */
/* sum of the (unsaturated) multiplicities held = k-mer occurrences inserted: the conservation check of a build */
int kmu_count_nb_occurrences(kmu_counter *c, uint64_t *out);
/* k-mers whose in-table count has reached kmu_count_table_info_t.count_ceiling (a homopolymer in a deep read set): for them the sum
 * above and a raw export are lower bounds -- an inexact total then reads "saturated", not "k-mers lost" */
int kmu_count_nb_saturated(kmu_counter *c, uint64_t *out);
/* The table in HBM (no counterpart upstream: the reference's filters size themselves, kmercount.rs:70-123).  Slots: whole regions
 * of 4096 -- capacity_hint / 0.70 of them, NOT rounded to a power of two (round 5: the image of a big table is written by every
 * partitioned build).  Big tables (more than 2048 regions whose index is worth >= 11 bits with 8-bit counters, >= 17 with 16-bit
 * ones) keep ONE 8-byte word per slot -- the bits of the table hash that the slot's position does not already say, and a count field of
 * count_field_bits that stops a little below its maximum (every reader saturates at 2^counter_bits - 1 like
 * kmercount.rs:1615; kmu_count_nb_occurrences is exact while no k-mer occurs 2^count_field_bits - 1024 times) --, small ones
 * a 64-bit key + a 32-bit count. */
typedef struct kmu_count_table_info_t {
    uint64_t nslots;
    uint64_t table_bytes;
    uint32_t bytes_per_slot;   /* 8 or 12 */
    uint32_t count_field_bits; /* width of the in-table count */
    uint64_t count_ceiling;    /* the largest count a slot holds: 2^32 - 1 (12-byte slots), 2^count_field_bits - 1024 (8-byte slots).  Queries saturate at 2^counter_bits - 1 long before;
                                  kmu_count_nb_occurrences and the raw counts of kmu_count_export_part are exact while
                                  kmu_count_nb_saturated is 0 */
} kmu_count_table_info_t;
int kmu_count_table_info(const kmu_counter *c, kmu_count_table_info_t *out);
/* dump of (canonical k-mer, count) for count >= min_count (dump_kmer_counter, kmercount.rs:500-525 uses 2).
 * Call with kmers_out == NULL to get the number of records in *n_out; records are sorted by k-mer value. */
int kmu_count_dump(kmu_counter *c, uint32_t min_count, uint64_t *kmers_out, uint32_t *counts_out, uint64_t cap,
                   uint64_t *n_out);
/* KmerCounter::eliminate_once_kmer (kmercount.rs:110-117): forget the k-mers seen once; counts >= 2 are kept */
int kmu_count_eliminate_once(kmu_counter *c);
/* The k-mers seen exactly once, with where they sit (KmerFilter1::dump_in_file_once_kmer16b32bit, kmercount.rs:1031-1082;
 * the `Unicity` branch of parsefastq): for every k-mer occurrence of the given reads, in (sequence, position) order, whose
 * canonical k-mer has count exactly 1 in the counter: canonical value, sequence number, k-mer rank in its sequence.
 * Unpacked (ASCII) input.  Call with kmers_out == NULL for the number of records in *n_out. */
int kmu_count_once_positions(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                             uint64_t *kmers_out, uint32_t *numseq_out, uint32_t *numkmer_out, uint64_t cap, uint64_t *n_out);
/* ---- reading the table back (no counterpart upstream: the reference's filters cannot be enumerated) ----
 * The count spectrum.  hist_out[v], v < n_bins: the number of distinct canonical k-mers held whose REPORTED count -- what
 * kmu_count_query answers: min(multiplicity, 2^counter_bits - 1) -- is v; the last bin collects every count >= n_bins - 1.
 * hist_out[0] is always 0 (an entry that left for its owner is absent for every reader).  2 <= n_bins <= 65536; bins above
 * 2^counter_bits - 1 stay 0.  A distributed counter answers for its own partition after kmu_count_finalize (owners are
 * disjoint: the ranks' arrays add up). */
int kmu_count_histogram(kmu_counter *c, uint64_t *hist_out, uint32_t n_bins, int mem);

typedef struct kmu_read_abundance { /* 32 bytes */
    uint32_t n_kmers;  /* L - k + 1; 0 when L < k (all other fields 0 then) */
    uint32_t n_absent; /* reported count 0 */
    uint32_t n_once;   /* reported count 1 */
    uint32_t n_solid;  /* reported count >= solid_min */
    uint16_t min, median, max; /* of the reported counts; median = the value of rank (n_kmers - 1) / 2 in ascending order */
    uint16_t reserved; /* 0 */
    uint64_t sum;      /* of the reported counts */
} kmu_read_abundance;

/* The abundance of the k-mers of reads in the table.  For every k-mer start p of every sequence i: the reported count of its
 * canonical k-mer.
 * counts_out (may be NULL): counts_out[offsets[i] + p], p in [0, L_i - k + 1) -- the layout of kmu_kmer_hashes, including
 *   offsets[0] != 0 and what happens to the last k - 1 positions of a sequence (untouched in device arrays, zero in host arrays).
 * stats_out (may be NULL): n_seq records.  At least one of the two must be given.
 * Unpacked (ASCII) input.  A sequence shorter than k gets the all-zero record; non-ACGT bytes are KMU_E_NON_ACGT as in
 * kmu_count_add_reads.  KMU_E_UNSUPPORTED: a counter distributed over more than one rank (its table holds only its own keys), a
 * sequence of 2^32 bases or more.  With stats_out alone the counts pass through a bounded workspace. */
int kmu_count_read_profile(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                           uint32_t solid_min, uint16_t *counts_out, kmu_read_abundance *stats_out);

/* ---- the count prefilter: a two-plane Bloom filter that keeps singletons off the table ---------------------------------------
 * The reference keeps the k-mers seen once in a cuckoo filter and counts the others in a counting Bloom filter
 * (src/base/kmercount.rs:70-123, :241-267); get_above2_count, dump_kmer_counter and the COUNTER_MULTIPLE file only ever ask for
 * counts >= 2.  The exact table costs 11.4 bytes per DISTINCT k-mer, most of them sequencing errors seen once.  A kmu_kfilter is
 * built in a first pass over the reads; a second pass (kmu_count_add_reads_filtered) counts only the k-mers the filter says may
 * occur twice.  Contract: every count in the table is exact; every k-mer that occurs at least twice is in the table; a k-mer that
 * is absent occurred 0 or 1 times.
 *
 * The structure (normative).  n_cells cells of 16 bytes {uint64 A, uint64 B}, n_cells in [1, 2^32 - 1], any value.  Modulo 2^64:
 *   sm(z):  z += 0x9E3779B97F4A7C15; z = (z ^ z>>30) * 0xBF58476D1CE4E5B9; z = (z ^ z>>27) * 0x94D049BB133111EB; return z ^ z>>31
 *   key v = the canonical compressed value as uint64;  h = sm(v);  g = sm(h)
 *   cell(v) = ((h >> 32) * n_cells) >> 32
 *   mask(v) = OR over i < n_hashes of 1 << ((g >> 6 i) & 63), 1 <= n_hashes <= 8 (coinciding positions collapse)
 * Adding one occurrence of v: old = atomic_or(&A[cell], mask); rep = old & mask; if (rep) atomic_or(&B[cell], rep).  The final
 * state is a function of the MULTISET of occurrences alone -- whatever the order, the launch shape or the number of add calls:
 * A[c] = the OR of the masks that landed in c, bit b of B[c] = "at least two occurrences landed on bit b of c".
 * The class of v: 0 -- some mask bit is missing in A: never added; 1 -- the mask is in A, not all of it in B: added exactly once;
 * 2 -- the mask is in B: may have been added twice or more.  A k-mer added at least twice is always class 2; class 2 for a k-mer
 * added once (or never) is the only error, at the Bloom rate of plane A (0.5 % of the singletons at 16 bits per distinct k-mer and
 * 4 hashes). */
typedef struct kmu_kfilter kmu_kfilter;
typedef struct kmu_kfilter_params {
    int32_t kmer_type;  /* a DNA k-mer type (amino acids: KMU_E_BAD_ARG) */
    int32_t kmer_size;
    uint32_t n_hashes;  /* 1 .. 8 */
    uint32_t flags;     /* 0 */
    uint64_t n_cells;   /* 1 .. 2^32 - 1: 16 bytes each (kmu_kfilter_cells_for) */
} kmu_kfilter_params;
typedef struct kmu_kfilter_info_t { /* 56 bytes */
    uint64_t n_cells, bytes;     /* bytes = 16 n_cells */
    uint32_t n_hashes, kmer_size;
    uint64_t n_added;            /* the occurrences added since the last reset (those of merged filters included) */
    uint64_t bits_a, bits_b;     /* set bits of the two planes */
    double est_distinct;         /* -(m / n_hashes) ln(1 - bits_a / m), m = 64 n_cells; INFINITY when plane A is full */
} kmu_kfilter_info_t;
/* plain host C, no device: max(1, ceil(expected_distinct * bits_per_kmer / 64)) cells; 0 when that exceeds 2^32 - 1 */
uint64_t kmu_kfilter_cells_for(uint64_t expected_distinct, uint32_t bits_per_kmer);
/* KMU_E_BAD_ARG: null pointers, n_hashes outside [1, 8], n_cells outside [1, 2^32 - 1], flags != 0, an amino-acid k-mer type; a
 * k-mer type and size that kmu_count_create refuses is refused the same way.  The filter starts empty. */
int kmu_kfilter_create(kmu_ctx *ctx, const kmu_kfilter_params *p, kmu_kfilter **out);
void kmu_kfilter_destroy(kmu_kfilter *f);
int kmu_kfilter_reset(kmu_kfilter *f); /* both planes and n_added back to 0 */
/* one occurrence of every canonical k-mer of every sequence.  Unpacked (ASCII) input only; non-ACGT bytes (KMU_E_NON_ACGT, the
 * planes are then unspecified), reads shorter than k, offsets[0] != 0 and n_seq == 0 exactly as in kmu_count_add_reads. */
int kmu_kfilter_add_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem);
/* one occurrence of each of n canonical compressed values */
int kmu_kfilter_add_kmers(kmu_kfilter *f, const uint64_t *canon_kmers, uint64_t n, int mem);
/* class_out[i] = 0 / 1 / 2, the class of canon_kmers[i] */
int kmu_kfilter_query(kmu_kfilter *f, const uint64_t *canon_kmers, uint64_t n, int mem, uint8_t *class_out);
/* the popcounts of the planes (one kernel, one synchronisation) and the cardinality estimate, computed in double on the host */
int kmu_kfilter_info(kmu_kfilter *f, kmu_kfilter_info_t *out);
/* words_out[2 n_cells]: A0 B0 A1 B1 ... */
int kmu_kfilter_export(kmu_kfilter *f, uint64_t *words_out, int mem);
/* dst becomes the filter of the concatenated input: A = A1 | A2, B = B1 | B2 | (A1 & A2), n_added the sum -- the hook for ranks
 * that each filtered a shard.  The two filters must share context and parameters (KMU_E_BAD_ARG otherwise, dst unchanged). */
int kmu_kfilter_merge(kmu_kfilter *dst, const kmu_kfilter *src);
/* The canonical k-mer of every class-2 occurrence of the given reads, in (sequence, position) order.  Call with kmers_out == NULL
 * for the number of k-mers in *n_out (host memory in both modes); cap < that number: KMU_E_BAD_ARG with *n_out set and nothing
 * written -- the rules of kmu_count_once_positions.  One synchronisation, for the total. */
int kmu_kfilter_select_reads(kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                             uint64_t *kmers_out, uint64_t cap, uint64_t *n_out);
/* Adds exactly the occurrences kmu_kfilter_select_reads lists to the counter; *n_passed_out (may be NULL): their number, by which
 * kmu_count_nb_occurrences has grown.  After a filter built from the same reads: every k-mer seen at least twice is held with its
 * exact count, and kmu_count_nb_unique counts the SINGLETONS THAT SLIPPED THROUGH the filter (its false positives), not the
 * singletons of the reads.  The survivors pass through a workspace of KMU_KFILTER_CHUNK_KMERS k-mers (default 2^26) into the
 * counter's own add of k-mer arrays, range by range.  KMU_E_BAD_ARG: a counter and a filter of different contexts, k-mer types or
 * sizes.  KMU_E_UNSUPPORTED: a distributed counter.  KMU_E_NON_ACGT is found before anything is added; a later failure
 * (KMU_E_TABLE_FULL) leaves the counter as a failed kmu_count_add_kmers does, *n_passed_out telling what went in before. */
int kmu_count_add_reads_filtered(kmu_counter *c, kmu_kfilter *f, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                                 int mem, uint64_t *n_passed_out);
/* multi-GPU merge (one process per GPU): export the entries whose owner (int64_hash(kmer) % n_parts,
 * kmercount.rs:412-420) is `part` as device/host arrays, and merge entries received from peers.
 * The exchange itself is done by the host layer (RCCL all_to_all over xGMI). */
int kmu_count_export_part(kmu_counter *c, uint32_t part, uint32_t n_parts, uint64_t *kmers_out, uint32_t *counts_out,
                          uint64_t cap, int mem, uint64_t *n_out);
int kmu_count_merge_entries(kmu_counter *c, const uint64_t *kmers, const uint32_t *counts, uint64_t n, int mem);
/* multi-GPU counting, the throughput path: the canonical k-mers of the reads grouped by owner rank
 * (`int64_hash(kmer) % n_parts`, the reference's own key-space dispatch, kmercount.rs:412-420,942).
 * *dev_kmers_out points to a device buffer owned by the counter's context (valid until its next call);
 * part_bounds_out[n_parts + 1] (host) delimits the group of every owner.  The caller exchanges the groups
 * (all-to-all over RCCL) and feeds what it receives to kmu_count_add_kmers. */
int kmu_count_extract_by_owner(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                                uint32_t n_parts, uint64_t **dev_kmers_out, uint64_t *part_bounds_out);
/* drop every entry not owned by `part` (after the exchange each rank keeps only its key range) */
int kmu_count_retain_part(kmu_counter *c, uint32_t part, uint32_t n_parts);

/* ---- multi-GPU: one rank per GPU, RCCL over xGMI ------------------------------------------------------------------
 * The reference's parallel drivers are threads of one process: count_kmer_threaded_one_to_many (src/base/kmercount.rs:881-974)
 * dispatches every canonical k-mer to the thread that owns it (`int64_hash(kmer) % n`, :412-420, :942) over channels, and
 * KmerCounterPool (:424-565) keeps one counter per thread; sketching is a rayon map over reads
 * (src/sketching/seqsketchjaccard.rs:245-248).  Here a rank is a GPU with its own kmu_ctx (one process per GPU, or one
 * thread per GPU), the channel is ONE all-to-all over xGMI inside the library, and sketching shards reads with no
 * collective.  Rank 0 creates an id and hands its 128 bytes to the other ranks by any means the host has (a file, MPI, a
 * socket, torch.distributed); every rank then calls kmu_comm_init (collective).  RCCL is bound when the first of these
 * calls is made, to the copy already mapped into the process if there is one. */
#define KMU_COMM_ID_BYTES 128
typedef struct kmu_comm_id { char bytes[KMU_COMM_ID_BYTES]; } kmu_comm_id; /* an ncclUniqueId */
int kmu_comm_get_id(kmu_comm_id *out);
int kmu_comm_init(kmu_ctx *ctx, const kmu_comm_id *id, int rank, int nranks);
/* A transport supplied by the host instead (a host that owns a communicator already; tests with more ranks than GPUs).
 * alltoallv (may be NULL: the library's COPY transport, below): device pointers; counts and displacements per peer in elements of elem_bytes; the library has synchronised
 * `stream` before the call and expects the received data to be visible to the device at return.  allgather: host memory,
 * `bytes` from every rank, rank order.  Both return 0 on success. */
typedef int (*kmu_alltoallv_fn)(void *user, const void *send_dev, const uint64_t *send_counts, const uint64_t *send_displs,
                                void *recv_dev, const uint64_t *recv_counts, const uint64_t *recv_displs, uint32_t elem_bytes,
                                void *stream);
typedef int (*kmu_allgather_fn)(void *user, const void *send_host, void *recv_host, uint64_t bytes);
int kmu_comm_init_custom(kmu_ctx *ctx, int rank, int nranks, kmu_alltoallv_fn alltoallv, kmu_allgather_fn allgather, void *user);
/* The COPY transport (round 5): the all-to-all of a distributed add as N - 1 device-to-device copies straight into the peers' receive
 * buffers -- mapped through HIP IPC (hipIpcGetMemHandle / hipIpcOpenMemHandle) when the peer is another process of this node, used as
 * they are when it is a thread of this one -- on the communicator's exchange stream.  No kernel of a collective library has to find
 * a CU under the persistent sketch kernels a step runs the exchange under (RCCL's send / receive kernels do: measured on one GPU,
 * profiles/r05_reserve.txt).  The communicator's all-gather (RCCL's, or the host's) carries the handles and closes the exchange with
 * a host barrier.  One node only.  kmu_comm_set_transport(ctx, KMU_TRANSPORT_COPY) switches an existing communicator over (every
 * rank alike, between exchanges); kmu_comm_init_custom with alltoallv == NULL creates one that has only this transport.  An exchange
 * for which some rank cannot export its receive buffer goes -- on every rank: all read the same published rows -- through the
 * communicator's other data path (RCCL, or the host's all-to-all) if it has one, and fails with KMU_E_RCCL otherwise. */
typedef enum kmu_transport { KMU_TRANSPORT_DEFAULT = 0 /* RCCL, or the host's all-to-all function */, KMU_TRANSPORT_COPY = 1 } kmu_transport;
int kmu_comm_set_transport(kmu_ctx *ctx, int transport);
int kmu_comm_transport(const kmu_ctx *ctx); /* kmu_transport of the context's communicator */
int kmu_comm_destroy(kmu_ctx *ctx); /* also done by kmu_destroy */
int kmu_comm_rank(const kmu_ctx *ctx);   /* -1 without a communicator */
int kmu_comm_nranks(const kmu_ctx *ctx); /* 0 without a communicator */
int kmu_comm_allgather(kmu_ctx *ctx, const void *send_host, void *recv_host, uint64_t bytes); /* host memory, collective */

/* Distributed counting.  A counter created with KMU_COUNT_DISTRIBUTED on a context that has a communicator is one member of
 * a KmerCounterPool spread over the ranks: kmu_count_add_reads takes THIS rank's reads (collective: every rank calls it,
 * with its own shard, possibly empty), kmu_count_finalize (collective) completes the exchange; afterwards rank r's counter
 * holds exactly the canonical k-mers with owner r with their multiplicities over ALL ranks' reads, and every query / dump /
 * statistic of this header sees that partition.
 * Who owns a k-mer (kmu_count_owner_kind; every rank of a pool must create its counter alike):
 *   KMU_OWNER_MINIMIZER  (default where a minimizer window fits: Kmer64bit, 17 <= k <= 31) the owner is a function of the k-mer's
 *                MINIMIZER -- the canonical m-mer of smallest hash among the k - m + 1 it contains (m = 9 .. 15 by k), the same on
 *                both strands: kmu_kmer_owner_minimizer.  Consecutive k-mers of a read mostly share it, so the occurrences travel
 *                as SUPER-K-MER RECORDS: a run of up to 16 consecutive k-mers with one owner as its 2-bit bases, 12 bytes, ~1.35 B
 *                per k-mer at k = 31 instead of one 8-byte message per k-mer (the reference's unit of dispatch, kmercount.rs:936-943).
 *   KMU_OWNER_HASH       (KMU_COUNT_OWNER_HASH, KMU_COUNT_OWNER=hash, and every k <= 16) the reference's own dispatch
 *                kmu_kmer_owner: int32_hash / int64_hash(kmer) % n, DispatchableT (kmercount.rs:382-420).
 * Routes, chosen per add from the measured duplication (occurrences / distinct k-mers, estimated on a hash sample of this batch
 * over all ranks) with a cost model (kmu_comm_stats; KMU_COUNT_ROUTE=occurrences|superkmers|merge forces one):
 *   OCCURRENCES  (hash owners) every k-mer occurrence travels to its owner (8 B each), the owner builds its table from what it
 *                receives: the reference's own dispatch.
 *   SUPERKMERS   (minimizer owners) the same with 12-byte records in place of k-mers; the owner expands them inside the first
 *                level of its partitioned build.
 *   MERGE        every rank counts its shard locally; at finalize the (k-mer, count) entries it does not own travel
 *                (12 B per DISTINCT k-mer) and are added to the owner's table: less traffic only once a k-mer occurs many times
 *                per rank (more than ~1.5 with hash owners, ~9 with minimizer owners), at the price of building twice. */
#define KMU_COUNT_DISTRIBUTED 0x1 /* kmu_count_params.flags */
#define KMU_COUNT_OWNER_HASH 0x2  /* with KMU_COUNT_DISTRIBUTED: owners by the reference's dispatch (kmu_kmer_owner) */
typedef enum kmu_owner_kind { KMU_OWNER_HASH = 0, KMU_OWNER_MINIMIZER = 1 } kmu_owner_kind;
typedef enum kmu_count_route { KMU_ROUTE_NONE = 0, KMU_ROUTE_OCCURRENCES = 1, KMU_ROUTE_MERGE = 2, KMU_ROUTE_SUPERKMERS = 3 } kmu_count_route;
typedef struct kmu_comm_stats {
    int32_t route;                 /* kmu_count_route of the last distributed kmu_count_add_reads */
    int32_t sample_shift;          /* the duplication was measured on the k-mers whose owner hash has this many zero bits */
    double dup_ratio;              /* occurrences / distinct over all ranks (sampled); 0 = not measured */
    uint64_t kmers_local;          /* k-mer occurrences of this rank's shard (last add) */
    uint64_t bytes_occurrences;    /* what OCCURRENCES / SUPERKMERS moves off this rank for that add: 8 B x the occurrences (12 B x
                                      the records) that other ranks own */
    uint64_t bytes_merge;          /* what MERGE moves off this rank: 12 B x distinct x (N-1)/N (from dup_ratio until
                                      finalize has run, exact afterwards) */
    uint64_t bytes_sent;           /* bytes that really left this rank / arrived, last add + its finalize */
    uint64_t bytes_received;
    double model_ms_occurrences;   /* the cost model's estimates the choice was made from (OCCURRENCES or SUPERKMERS; MERGE) */
    double model_ms_merge;
    int32_t owner_kind;            /* kmu_owner_kind of the counter of the last add */
    int32_t exchanges;             /* all-to-alls of the last add + its finalize */
    uint64_t records_local;        /* super-k-mer records of this rank's shard (0 with hash owners) */
    double exchange_ms;            /* MEASURED duration of those all-to-alls: events around them on the exchange stream (RCCL), wall
                                      time of the host's function (kmu_comm_init_custom).  An exchange still in flight is counted by the next query. */
    double exchange_gbps_out;      /* bytes_sent / exchange_ms and bytes_received / exchange_ms, in GB/s: the link rate the route */
    double exchange_gbps_in;       /* model assumes as KMU_XGMI_GBPS */
} kmu_comm_stats;
int kmu_comm_get_stats(const kmu_ctx *ctx, kmu_comm_stats *out);
int kmu_count_finalize(kmu_counter *c);
int kmu_count_owner_kind(const kmu_counter *c); /* kmu_owner_kind of a distributed counter (KMU_OWNER_HASH for any other) */
/* owner of canonical k-mer values in an n_parts-way pool: int32_hash / int64_hash(kmer) % n_parts by the width of the
 * k-mer type (Kmer32bit / Kmer16b32bit: kmercount.rs:386-402; Kmer64bit :412-420).  Host arithmetic, no device needed. */
int kmu_kmer_owner(int kmer_type, const uint64_t *canon_kmers, uint64_t n, uint32_t n_parts, uint32_t *owners_out);
/* the minimizer owner of Kmer64bit values of kmer_size bases (17 .. 31; forward or canonical value: both strands agree).  Host
 * arithmetic, no device needed. */
int kmu_kmer_owner_minimizer(int kmer_size, const uint64_t *canon_kmers, uint64_t n, uint32_t n_parts, uint32_t *owners_out);
/* The two halves of the SUPERKMERS route for hosts that run the exchange themselves (kmu_count_extract_by_owner's counterpart).
 * A record is 12 bytes = three uint32: up to 46 bases, 2 bits each, the first in bits 31..30 of word 0, zeros behind the last;
 * bits 3..0 of word 2 = number of k-mers - 1 (1 .. 16 k-mers: consecutive k-mers of one read with one minimizer owner).
 * kmu_count_extract_superkmers: the records of the reads grouped by owner; *dev_records_out points to a device buffer owned
 * by the counter's context (valid until its next call), record_bounds_out[n_parts + 1] (host, in records) delimits the group of
 * every owner, kmers_per_part_out[n_parts] (host, may be NULL) says how many k-mers each group holds.
 * kmu_count_add_superkmers: the k-mers of n_records records into the table (KMU_MEM_DEVICE or KMU_MEM_HOST). */
int kmu_count_extract_superkmers(kmu_counter *c, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                                 uint32_t n_parts, void **dev_records_out, uint64_t *record_bounds_out, uint64_t *kmers_per_part_out);
int kmu_count_add_superkmers(kmu_counter *c, const void *records, uint64_t n_records, int mem);

/* ---- L-1 ingest: the step before the path ----------------------------------------------------
 * FASTQ / FASTA text -> the accepted reads as (bases, offsets), in file order.  kmu_ingest_fastq: 4-line records,
 * "\n" or "\r\n".
 * Rule of the reference's readers: a record with any byte outside ACGTacgt is dropped and counted
 * (readblockseq, src/bin/datasketcher.rs:358-388; parse_with_needletail, src/io.rs:37-57).
 * Call with bases_out == offsets_out == NULL to get the sizes in *info, then with buffers of at least
 * info->kept_bases bytes and info->n_kept + 1 offsets.  record_index_out (optional, n_kept entries) = position of every
 * kept read among the records of the text.  `text` must be 16-byte aligned in KMU_MEM_DEVICE mode.
 * Errors: KMU_E_BAD_ARG for a malformed or truncated record (the reference: `record.expect("invalid record")`). */
typedef struct kmu_ingest_info {
    uint64_t n_records;    /* records in the text */
    uint64_t n_kept;       /* records made of ACGTacgt only */
    uint64_t kept_bases;   /* sum of their lengths */
    uint64_t n_bases;      /* bases of all records        (io.rs:40) */
    uint64_t nb_bad_bases; /* non-ACGT bytes in sequences (io.rs:42) */
    uint64_t nb_bad_reads; /* dropped records             (io.rs:47, datasketcher.rs:368) */
} kmu_ingest_info;
int kmu_ingest_fastq(kmu_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint8_t *bases_out, uint64_t bases_cap,
                     uint64_t *offsets_out, uint64_t offsets_cap, uint32_t *record_index_out, kmu_ingest_info *info);

/* FASTA, needletail's other format (what gsearch feeds): a line that starts with '>' opens a record; its sequence is the
 * following lines up to the next such line with the line ends removed (record.seq()).  The last line may have no final newline,
 * and a '\r' that ends the text is dropped like one before a newline.  Same rule, outputs and calling convention as
 * kmu_ingest_fastq.  KMU_E_BAD_ARG if the text does not start with '>'. */
int kmu_ingest_fasta(kmu_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint8_t *bases_out, uint64_t bases_cap,
                     uint64_t *offsets_out, uint64_t offsets_cap, uint32_t *record_index_out, kmu_ingest_info *info);
/* needletail::parse_fastx_file (src/io.rs:37, src/bin/datasketcher.rs:211): the first byte names the format,
 * '>' FASTA, '@' FASTQ; anything else is KMU_E_BAD_ARG.  (Compressed input is not handled: decompress first.) */
int kmu_ingest_fastx(kmu_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint8_t *bases_out, uint64_t bases_cap,
                     uint64_t *offsets_out, uint64_t offsets_cap, uint32_t *record_index_out, kmu_ingest_info *info);
/* kmu_ingest_fastq that keeps the quality line: everything kmu_ingest_fastq returns is the same byte for byte (the sizes-only
 * call with every output NULL included), and quals_out[offsets_out[i] + p] is the raw quality byte of base p of kept read i
 * (quals_cap >= info->kept_bases; bases_out, quals_out and offsets_out go together).  The quality line starts after the newline
 * that ends the separator line and ends at the next newline (a '\r' before it is dropped; the last record may have no final
 * newline, and a '\r' that ends the text is dropped the same way).  A record -- kept or dropped -- whose quality line differs in length from its sequence is KMU_E_BAD_ARG ("invalid
 * record": needletail refuses such a file), found before any output is written. */
int kmu_ingest_fastq_qual(kmu_ctx *ctx, const uint8_t *text, uint64_t n_bytes, int mem, uint8_t *bases_out, uint64_t bases_cap,
                          uint8_t *quals_out, uint64_t quals_cap, uint64_t *offsets_out, uint64_t offsets_cap,
                          uint32_t *record_index_out, kmu_ingest_info *info);

/* ---- read statistics: the base and quality distributions of a batch -----------------------------------
 * Reference: get_base_count_par (src/statutils.rs:229-347) -- the read-length histogram and the table of per-read base
 * percentages that parsefastq writes as readlen.histo and bases.histo -- and remap_quality8 (src/quality/quality.rs:33-43).
 * Integers only; every output is a pure function of the input (integer atomics that commute), whatever the launch shape.
 *   class of a base byte   A/a 0, C/c 1, G/g 2, T/t 3, every other byte (N, '\n', 0x00, 0xFF, ...) "other"
 *   pct of base b          (200 h + L) / (2 L) in integer division for a read of L bases with h of b; 0 for L == 0.  This is
 *                          ((100 * h) as f64 / L as f64).round() of statutils.rs:255-256: ties go up (L 8, h 1: 13)
 *   length bucket          HdrHistogram's layout of Histogram::new_with_bounds(1, max_len, sig_digits), statutils.rs:67:
 *                          sub_bits = ceil(log2(2 * 10^sig_digits)) (5, 8, 11, 15, 18 for 1 .. 5), half = 2^(sub_bits - 1),
 *                          shift = max(0, floor(log2(len)) - (sub_bits - 1)) (0 for len 0), bucket = shift * half + (len >> shift).
 *                          ranges = the smallest j >= 1 with 2^sub_bits * 2^(j - 1) > max_len, limit = 2^sub_bits << (ranges - 1),
 *                          n_buckets = (ranges + 1) * half; a length >= limit has no bucket and is counted in histo_out
 *                          (record_read_len, statutils.rs:193-199).  max_len 1 000 000, sig_digits 3: limit 1 048 576 and
 *                          11 264 buckets.  The lowest length of a bucket is (bucket - shift * half) << shift with
 *                          shift = max(0, bucket / half - 1), its highest that + 2^shift - 1.
 *   quality class          0 for q < 0x25, else min(7, 1 + (q - 0x25) / 3): remap_quality8's f32 expression on all 256 bytes */
typedef struct kmu_read_comp {   /* 48 bytes */
    uint64_t n_base[4];          /* A C G T, either case */
    uint64_t n_other;
    uint8_t  pct[4];             /* as defined above */
    uint32_t len_bucket;         /* 0xFFFFFFFF when the length is >= limit */
} kmu_read_comp;
typedef struct kmu_read_stats_params { /* 16 bytes */
    int32_t  sig_digits;         /* 1 .. 5 */
    int32_t  flags;              /* 0 */
    uint64_t max_len;            /* > 0 */
} kmu_read_stats_params;
typedef struct kmu_read_stats_info {  /* 96 bytes */
    uint64_t n_reads, n_bases, n_base[4], n_other;
    uint64_t n_empty;            /* reads of length 0 */
    uint64_t histo_out;          /* reads with a length >= limit */
    uint64_t min_len, max_len;   /* over the reads of the batch; both 0 for n_reads == 0 */
    uint64_t n_buckets;
} kmu_read_stats_info;
typedef struct kmu_read_qual {   /* 80 bytes */
    uint64_t n_class[8];
    uint64_t sum_q;              /* sum of the raw bytes */
    uint8_t  min_q, max_q, median_class, pad[5]; /* min 0xFF / max 0 / median 0 for an empty read;
                                    median_class = smallest c with 2 * (n_class[0..c] summed) >= len */
} kmu_read_qual;
/* the layout of a length histogram and the range of one of its buckets; no device, no context.  KMU_E_BAD_ARG: sig_digits
 * outside 1 .. 5, max_len == 0, a null output. */
int kmu_len_hist_layout(uint64_t max_len, int sig_digits, uint32_t *n_buckets, uint64_t *limit);
int kmu_len_bucket_range(int sig_digits, uint32_t bucket, uint64_t *lowest, uint64_t *highest);
/* The statistics of the reads offsets[0 .. n_seq] of `bases` (unpacked bytes; offsets[0] need not be 0 nor aligned: the batch may
 * be a range of a larger one).  comp_out [n_seq], pct_hist [101][4] and len_hist [n_buckets] may each be NULL; info (host memory
 * in both modes) is required.  pct_hist[p * 4 + b] = the reads whose base b sits at percentage p (an empty read: row 0; every
 * read adds 4 to the table); len_hist[bucket] = the reads of that bucket.  The call owns its outputs: it zeroes them itself (a
 * second call into the same buffers gives the same values; device buffers may hold anything on entry).  n_seq == 0 is valid.
 * KMU_MEM_DEVICE: every array except p and info is device memory, `bases` 16-byte aligned; the call synchronises the stream once,
 * to hand info over (also in async_device contexts).  KMU_MEM_HOST: through the context's workspace.
 * KMU_E_BAD_ARG, nothing is written: null ctx / p / info / offsets, null bases with n_seq > 0, sig_digits outside 1 .. 5,
 * max_len == 0, flags != 0, bad mem. */
int kmu_read_stats(kmu_ctx *ctx, const kmu_read_stats_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq, int mem,
                   kmu_read_comp *comp_out, uint64_t *pct_hist, uint64_t *len_hist, kmu_read_stats_info *info);
/* classes_out[i] = the quality class of quals[i]; classes_out == quals is allowed.  KMU_E_BAD_ARG: null ctx, null arrays with n > 0,
 * bad mem. */
int kmu_quality_remap(kmu_ctx *ctx, const uint8_t *quals, uint64_t n, int mem, uint8_t *classes_out);
/* The same walk over the quality bytes of a batch (kmu_ingest_fastq_qual's quals_out with its offsets): out [n_seq] and class_hist
 * [8] (the batch totals per class) may each be NULL; both are zeroed by the call.  Memory as in kmu_read_stats; the call ends as
 * every other (no synchronisation of a KMU_MEM_DEVICE call in an async_device context).  KMU_E_BAD_ARG: null ctx / offsets, null
 * quals with n_seq > 0, bad mem. */
int kmu_read_qual_stats(kmu_ctx *ctx, const uint8_t *quals, const uint64_t *offsets, uint32_t n_seq, int mem, kmu_read_qual *out,
                        uint64_t *class_hist);

/* ---- L4 signature comparison: what the callers do with the signatures next --------------------
 * Rows are compared as raw words (4 bytes for KMU_SIG_U32 / F32, 8 for U64 / F64).
 * out[p] = number of slots t with A[ia[p]][t] == B[ib[p]][t]:
 *   probminhash_get_jaccard_objects (src/sketching/seqsketchjaccard.rs:86-108): jaccard = out / m
 *   DistBlockSketched::eval / distance_jaccard_serial (src/sketching/seqblocksketch.rs:419-440): (m - out) / m, and 1.0
 *   when both blocks belong to the same sequence (the caller's rule); DistHamming of datasketcher.rs:156-185 likewise.
 * sig_a has na rows of m words, sig_b nb rows (they may be the same array). */
int kmu_sig_equal_pairs(kmu_ctx *ctx, const void *sig_a, uint32_t na, const void *sig_b, uint32_t nb, uint32_t m,
                        int sig_type, const uint32_t *ia, const uint32_t *ib, uint64_t n_pairs, int mem, uint32_t *out);
/* all pairs: out[i * nb + j] (m <= 65535) */
int kmu_sig_equal_matrix(kmu_ctx *ctx, const void *sig_a, uint32_t na, const void *sig_b, uint32_t nb, uint32_t m,
                         int sig_type, int mem, uint16_t *out);
/* Exact k nearest neighbours: what `datasketcher ... ann --nb N` asks of an HNSW index under DistHamming /
 * DistBlockSketched (src/bin/datasketcher.rs:98-109, 137-192, 261-309), by brute force with the selection fused
 * behind the compare (no nq x ndb intermediate: nq x ndb may be far beyond memory).
 *   eq(i, j) = number of slots t < m with Q[i][t] == DB[j][t] (raw words, as above); distance = (m - eq) / m.
 *   Candidates of query i: every j < ndb, except -- when groups are given -- those with group_q[i] == group_db[j]
 *   (DistBlockSketched's rule, seqblocksketch.rs:419-440: blocks of one sequence are never paired; a self-join of
 *   whole-read signatures passes group = 0, 1, 2, ... on both sides so that a row is not its own neighbour).
 *   idx_out[i * k ..], eq_out[i * k ..]: the min(k, #candidates) best candidates by eq DESCENDING, then j ASCENDING
 *   (the same rule decides who enters at the k-th place); the remaining entries are idx = KMU_KNN_NONE, eq = 0.
 *   Candidates with eq == 0 are candidates like any other.  The result is a pure function of the inputs.
 * KMU_E_BAD_ARG: null pointer, m == 0, k == 0, bad sig_type, one group array without the other.
 * KMU_E_UNSUPPORTED: m > 65535, k > KMU_KNN_MAX_K, ndb == 0xFFFFFFFF.  nq == 0: KMU_OK; ndb == 0: lists of "none". */
#define KMU_KNN_MAX_K 64
#define KMU_KNN_NONE 0xFFFFFFFFu /* idx of a list entry that does not exist */
int kmu_sig_knn(kmu_ctx *ctx, const void *sig_q, uint32_t nq, const void *sig_db, uint32_t ndb, uint32_t m, int sig_type,
                uint32_t k, const uint32_t *group_q, const uint32_t *group_db, int mem, uint32_t *idx_out,
                uint16_t *eq_out);
/* minhash_distance / mininvhash_distance (src/sketching/minhash.rs:134-190, :295-340) on KMU_ALGO_BOTTOMK rows
 * (ascending hashes, u64::MAX padding).  out[3p..3p+2] = common, total, i: jaccard = common / total,
 * containment = common / i (MinHashDist). */
int kmu_minhash_distance_pairs(kmu_ctx *ctx, const uint64_t *hashes_a, uint32_t na, const uint64_t *hashes_b, uint32_t nb,
                               uint32_t m, const uint32_t *ia, const uint32_t *ib, uint64_t n_pairs, int mem,
                               uint32_t *out);
/* Anchor matching: the pairs of bottom-k rows that share one of their smallest hashes, with the distance of every pair -- the
 * join behind the reference's inverse index smallest hash -> (readnum, slicepos) (redis_dump, src/anchor.rs:187-197; MINHASH_1 is
 * n_keys = 1) and mininvhash_distance on what it finds, without the rows leaving the device.
 *   Rows (hashes_q: nq x m, hashes_db: ndb x m, possibly the same array) hold ascending distinct hashes padded with UINT64_MAX, as
 *   kmu_read_anchors and kmu_sketch(KMU_ALGO_BOTTOMK) write them; they are trusted to have that shape, as
 *   kmu_minhash_distance_pairs trusts them.  n(r) = the entries of row r in front of its padding.
 *   keys(r) = the first min(n_keys, n(r)) hashes of row r.  The padding is never a key: an empty row matches nothing.
 *   Candidates: (a in q, b in db) with keys(a) and keys(b) intersecting and, when groups are given, group_q[a] != group_db[b]
 *   (DistBlockSketched's rule, as in kmu_sig_knn: slices of one read are never paired).  A self-join passes the same array twice
 *   with group = read of the row and gets (a, b) and (b, a) both.
 *   Distance of a candidate: the triple (common, total, i) of kmu_minhash_distance_pairs for (row a first, row b second), bit for
 *   bit, early stop and top-up rules included -- common may be 0 (the walk stops after n(a) steps).
 *   Reported: the candidates with common >= min_common (0: all of them), each ONCE, under h* = min(keys(a) & keys(b)) -- which is
 *   also the smallest hash the two rows share at all.  Order: a ascending, then h*, then b.  A pure function of the inputs.
 *   *n_out (host memory in both modes) is always the total number of pairs.  pairs_out == NULL: nothing else is written (the
 *   count-only call).  Otherwise pairs_out[2p..] = (a, b) and, unless dist_out is NULL, dist_out[3p..] = common, total, i;
 *   cap < total: KMU_E_BAD_ARG with *n_out set and the outputs unspecified (the rule of kmu_count_dump).
 * KMU_MEM_DEVICE: every array except n_out is device memory; the call synchronises the stream once, to hand n_out over (also in
 * async_device contexts), as kmu_read_anchors reads its row count.
 * KMU_E_BAD_ARG: null ctx / hashes / n_out, m == 0, n_keys == 0 or > m, one group array without the other.
 * KMU_E_UNSUPPORTED: m > KMU_ANCHOR_MAX_NBKMER, ndb * n_keys >= 2^32.  nq == 0 or ndb == 0: KMU_OK, *n_out = 0.
 * How: the ndb * n_keys (key, row) entries are sorted by key on the device (a stable 8-bit LSD radix sort, one wave per tile of
 * KMU_ANCHOR_SORT_TILE entries and pass); one wave per query row then looks its keys up and walks each bucket 64 candidates at a
 * time, once to count and once to write.  One wave owns a whole bucket: a key shared by very many rows is slow and gives
 * quadratic output (no repeat mask here: kmu_anchor_index_match has one). */
#define KMU_ANCHOR_SORT_TILE 1024 /* entries one workgroup ranks per radix pass */
int kmu_anchor_match(kmu_ctx *ctx, const uint64_t *hashes_q, uint32_t nq, const uint64_t *hashes_db, uint32_t ndb, uint32_t m,
                     uint32_t n_keys, uint32_t min_common, const uint32_t *group_q, const uint32_t *group_db, int mem,
                     uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap, uint64_t *n_out);
/* Read overlaps: from the window pairs of kmu_anchor_match to read pairs -- which reads overlap, on which strand, at which
 * relative offset, with how much support -- by a vote over diagonals, without the pairs leaving the device.
 *   pairs[2p..] = (a, b) and dist[3p..] = (common, total, i) exactly as kmu_anchor_match writes them, in any order: the result
 *   does not depend on the order of the input.  dist == NULL: every pair weighs 1; otherwise the weight of pair p is dist[3p]
 *   (common).  row_offsets_q / row_offsets_db (n_reads + 1 entries each) are the arrays of kmu_anchor_layout, possibly the same
 *   array (a self-join).  Row a belongs to the read i with row_offsets_q[i] <= a < row_offsets_q[i + 1] and
 *   slice_a = a - row_offsets_q[i]; the same for b on the db side.  The offsets are trusted to be ascending; a row at or beyond the
 *   last offset is undefined input, as bad rows are in kmu_minhash_distance_pairs.
 *   Integer arithmetic only, a pure function of the inputs:
 *   For a read pair (A, B) and a strand s in {0 .. strands - 1}, every window pair of (A, B) has a diagonal:
 *   d = slice_a - slice_b for s = 0, d = slice_a + slice_b for s = 1.
 *   W_s(d) is the sum of the weights on diagonal d, V_s(d) the number of window pairs on it.
 *   For every occupied diagonal (V > 0) the band score is S_s(d) = sum of W_s(e) over e = d .. d + band.
 *   The winner of (A, B) is the (s, d) with the largest S; ties go to s = 0 before s = 1, then to the smallest d.
 *   The winner's record: diag = d, score = min(S, 2^32 - 1), votes = sum of V over the band, slice_a_min / slice_a_max over the
 *   window pairs in the band.
 *   Reported: one record per read pair that has at least one window pair, whose score is >= min_score and, under KMU_OVL_UPPER,
 *   whose read_a < read_b (a self-join: each pair once).  Order: read_a ascending, then read_b.
 *   band is there because two reads cut their windows at unrelated phases, so one true overlap lands on two neighbouring
 *   diagonals; band = 0 is the plain vote per diagonal.  strands = 2 is for strand-independent anchors (KMU_FHASH_CANON_VALUE),
 *   strands = 1 for the reference's forward anchors.
 *   *n_out (host memory in both modes) is always the total number of records.  out == NULL: nothing else is written (the
 *   count-only call).  cap < total: KMU_E_BAD_ARG with *n_out set and out unspecified.
 * KMU_MEM_DEVICE: every array except n_out is device memory; the call synchronises the stream once, to hand n_out over (also in
 * async_device contexts).  The row offsets are then read on the device and a refusal because of them comes at that point.
 * KMU_E_BAD_ARG: null ctx / pairs / offsets / n_out, strands not 1 or 2, unknown flag bits, pairs but n_reads_q or n_reads_db == 0.
 * KMU_E_UNSUPPORTED: band > KMU_OVL_MAX_BAND, n_pairs * strands >= 2^32, a last row offset >= 2^31 or, with strands = 2, the two
 * last offsets above 2^31 together (both kinds of diagonal must fit the biased 32-bit field and the int32 of the record).
 * n_pairs == 0: KMU_OK, *n_out = 0, nothing else is written.
 * How: one entry per window pair and strand, sorted by (read_a, read_b, strand, diagonal) with two stable radix sorts (the
 * diagonal key first, then the read pair; the passes of bytes that are the same in every key are skipped); equal keys are a run,
 * reduced by one wave; one wave per read pair then takes the band sums of its runs and the first largest, once to count and once
 * to write. */
#define KMU_OVL_MAX_BAND 8
#define KMU_OVL_UPPER 1u          /* flags: keep only read pairs with read_a < read_b (self-join: each pair once) */
typedef struct {                  /* 32 bytes */
    uint32_t read_a, read_b;      /* index into row_offsets_q / row_offsets_db */
    uint32_t strand;              /* 0: same strand (diag = slice_a - slice_b); 1: opposite (diag = slice_a + slice_b) */
    int32_t  diag;                /* first diagonal of the winning band, in slices */
    uint32_t score;               /* sum of weights in the band, clamped to UINT32_MAX */
    uint32_t votes;               /* number of matched window pairs in the band */
    uint32_t slice_a_min, slice_a_max; /* over the window pairs in the band */
} kmu_overlap;
int kmu_anchor_overlaps(kmu_ctx *ctx, const uint32_t *pairs, const uint32_t *dist, uint64_t n_pairs,
                        const uint64_t *row_offsets_q, uint32_t n_reads_q, const uint64_t *row_offsets_db, uint32_t n_reads_db,
                        uint32_t strands, uint32_t band, uint32_t min_score, uint32_t flags, int mem,
                        kmu_overlap *out, uint64_t cap, uint64_t *n_out);

/* Anchor index: the database side of kmu_anchor_match as an object -- built once, kept on the device, matched against by any
 * number of query batches (the reference's persistent inverse index, redis_dump, src/anchor.rs:187-197) -- with a repeat mask.
 *   kmu_anchor_index_create: ndb bottom-k rows of length m (trusted as kmu_anchor_match trusts them), a fixed n_keys and optional
 *   groups.  keys(b) = the first min(n_keys, n(b)) hashes of row b; the padding is never a key.  occ(h) = the number of database
 *   rows b with h in keys(b); query rows never count towards it.  The index owns device copies of the rows and the groups (its own
 *   allocations, not the context's workspace): the caller's arrays may be freed or overwritten once the call returns, any other
 *   library call may run between two matches, and the index is destroyed before its context, like a kmu_counter.  The call may
 *   synchronise.  ndb == 0 is a valid index that matches nothing.
 *   kmu_anchor_index_match: nq query rows of the index's m.  A hash h is MASKED iff max_occ > 0 and occ(h) > max_occ.
 *   U(a, b) = the hashes of keys(a) & keys(b) that are not masked.  Candidates: the pairs (a, b) with U(a, b) not empty and, with
 *   groups, group_q[a] != group_db[b].  Distance: the triple of kmu_minhash_distance_pairs over the WHOLE rows, bit for bit -- the
 *   mask decides only which pairs are seeded, never what a walk sees.  Reported: the candidates with common >= min_common, each
 *   once, under h* = min U(a, b).  Order: a ascending, then h*, then b.  Under a mask h* is NOT "the smallest hash the two rows
 *   share at all": the rows may share smaller hashes that are masked.  max_occ == 0 gives exactly the pairs, triples and order of
 *   kmu_anchor_match with the same arguments, and so does any max_occ >= the largest occupancy.  *n_out, the count-only call
 *   (pairs_out == NULL), the cap rule and the one synchronisation of a KMU_MEM_DEVICE call are those of kmu_anchor_match.
 *   kmu_anchor_index_occupancy: hist_out[c], c < n_bins, = the number of distinct keys with occupancy c; the last bin collects
 *   every occupancy >= n_bins - 1; hist_out[0] is 0; 2 <= n_bins <= 65536 (the conventions of kmu_count_histogram).
 *   kmu_anchor_index_info: sizes; n_entries = the sum of |keys(b)|, n_distinct = the distinct keys, max_occupancy = the largest occ.
 * KMU_E_BAD_ARG: null ctx / index / hashes / out / n_out, m == 0, n_keys == 0 or > m, bad mem, bad n_bins, group_q given where the
 * index has no groups or missing where it has.  KMU_E_UNSUPPORTED: m > KMU_ANCHOR_MAX_NBKMER, ndb * n_keys >= 2^32.
 * How: the sorted (key, row) entries of kmu_anchor_match, then a directory of the distinct keys (ukeys[d], ubeg[d]: the first
 * entry of the bucket) so that an occupancy is a subtraction; the sorted keys are dropped.  A match looks the keys of a query row
 * up one lane per key, by one binary search in the directory, and never touches the bucket of a masked key. */
typedef struct kmu_anchor_index kmu_anchor_index;
typedef struct {
    uint32_t ndb, m, n_keys, has_groups;
    uint64_t n_entries;      /* sum of |keys(b)| */
    uint64_t n_distinct;     /* distinct keys */
    uint32_t max_occupancy, pad;
    uint64_t device_bytes;   /* device memory the index owns */
} kmu_anchor_index_info_t;
int kmu_anchor_index_create(kmu_ctx *ctx, const uint64_t *hashes_db, uint32_t ndb, uint32_t m, uint32_t n_keys,
                            const uint32_t *group_db /* or NULL */, int mem, kmu_anchor_index **out);
void kmu_anchor_index_destroy(kmu_anchor_index *ix); /* NULL: no-op */
int kmu_anchor_index_info(const kmu_anchor_index *ix, kmu_anchor_index_info_t *out);
int kmu_anchor_index_occupancy(kmu_anchor_index *ix, uint64_t *hist_out, uint32_t n_bins, int mem);
int kmu_anchor_index_match(kmu_anchor_index *ix, const uint64_t *hashes_q, uint32_t nq, const uint32_t *group_q,
                           uint32_t min_common, uint32_t max_occ, int mem, uint32_t *pairs_out, uint32_t *dist_out, uint64_t cap,
                           uint64_t *n_out);

/* Connected components: from edges between items -- the kmu_overlap records of kmu_anchor_overlaps, the pairs of kmu_anchor_match,
 * the neighbour lists of kmu_sig_knn -- to which items belong together, without the edges leaving the device.
 *   Graph: undirected, over the nodes 0 .. n_nodes - 1.
 *   kmu_components: edge e is the record edges[e * stride .. e * stride + stride - 1] (uint32 words, e * stride in 64 bits): u = word 0,
 *   v = word 1.  weight_at == 0: every edge counts.  Otherwise 2 <= weight_at < stride and the edge counts iff word weight_at >=
 *   min_weight.  Pairs of kmu_anchor_match: stride 2, weight_at 0; kmu_overlap records: stride 8, weight_at 4 (score) or 5 (votes).
 *   kmu_components_knn: the lists of a kmu_sig_knn self-join (nq == ndb == n_nodes): edge (i, idx[i * k + j]) counts iff
 *   eq[i * k + j] >= min_eq; eq == NULL (min_eq must then be 0): every edge counts.
 *   An edge that does not count is skipped, and so is a self loop (u == v).  An edge with an endpoint >= n_nodes is skipped and never
 *   used as an index (KMU_KNN_NONE entries fall out by this rule): no input makes a kernel read or write out of bounds.  Duplicate
 *   edges and edges given in both directions change nothing.
 *   label_out[v] (n_nodes entries, required): the smallest node of v's component.
 *   cluster_out[v] (n_nodes entries, or NULL): the number of components whose smallest node is below label_out[v] -- dense ids
 *   0 .. n_components - 1 in the order of the smallest member.
 *   size_out[c] (n_nodes entries, or NULL): the size of cluster c for c < n_components, 0 from there on.
 *   members_out (n_nodes entries, or NULL): the nodes ordered by (cluster, node); cluster c occupies the entries from the exclusive
 *   prefix sum of size_out.
 *   *n_components_out (host memory in both modes, or NULL): the number of components.
 *   A pure function of the inputs: the result does not depend on the order of the edges, on the launch shape or on timing.
 * n_nodes == 0: KMU_OK, 0 components, no array is written.  n_edges == 0: every node is its own cluster.
 * KMU_MEM_DEVICE: every array except n_components_out is device memory.  The count is the only thing that has to cross to the
 * host: with n_components_out the call synchronises the stream once to hand it over (also in async_device contexts); with NULL an
 * async_device context enqueues and returns, which is how a pipeline keeps going.  KMU_MEM_HOST: the inputs go up through the
 * context's workspace and the results come back, as in kmu_anchor_overlaps.
 * KMU_E_BAD_ARG: null ctx / label_out, null edges with n_edges > 0 (null idx with n_nodes > 0), stride < 2, weight_at == 1 or
 * >= stride, k == 0 with n_nodes > 0, null eq with min_eq > 0, bad mem.  KMU_E_UNSUPPORTED: n_nodes == 0xFFFFFFFF.
 * How: a lock-free union-find with label_out as the parent array.  One lane per edge finds the roots of both ends (relaxed
 * agent-scope atomic loads, path halving), leaves if they are equal -- once a component has formed most of its edges touch no root
 * with an atomic -- and otherwise hooks the LARGER root under the SMALLER by compare-and-swap; a lane that loses the race goes on
 * with the value it saw, so no lane ever waits for another.  parent[v] <= v holds throughout and entries only decrease: the root a
 * component ends with is its smallest node, whoever won which race.  Then every node takes its root; the roots are flagged and
 * scanned for the dense numbers; sizes are integer atomic adds; the member lists are a stable radix sort of (cluster, node). */
int kmu_components(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *edges, uint64_t n_edges, uint32_t stride,
                   uint32_t weight_at, uint32_t min_weight, int mem,
                   uint32_t *label_out, uint32_t *cluster_out, uint32_t *size_out, uint32_t *members_out,
                   uint32_t *n_components_out);
int kmu_components_knn(kmu_ctx *ctx, uint32_t n_nodes, const uint32_t *idx, const uint16_t *eq, uint32_t k, uint32_t min_eq,
                       int mem, uint32_t *label_out, uint32_t *cluster_out, uint32_t *size_out, uint32_t *members_out,
                       uint32_t *n_components_out);

/* ---- window minimizers: the (w, k) minimizers of every read, selected on the device ---------------------------------
 * Read i has L bases and nk = max(0, L - k + 1) k-mers.  h(p), p in [0, nk), is exactly the value kmu_kmer_hashes writes at
 * out[offsets[i] + p] for the same kmu_hash_params: 64-bit, zero-extended for the u32 types, p->fhash applied.
 * Windows (only when nk > 0): window j covers the positions [j, min(j + w, nk)) for j = 0 .. max(nk - w, 0); a read with
 *   1 <= nk <= w has the single window of all its k-mers; a read with nk == 0 has no window, no minimizer and is no error.
 * Selection: the minimizer of a window is its position of smallest h; TIES GO TO THE SMALLEST POSITION.  The minimizers of a
 *   read are the distinct positions its windows choose.  With this tie rule the chosen position never decreases from one window
 *   to the next, so "distinct" is "differs from the previous window's choice" and the result is strictly ascending in position.
 * Outputs: the minimizers of all reads, concatenated in read order, in position order within a read;
 *   mini_offsets_out[i] .. mini_offsets_out[i + 1] are the entries of read i.  Entry e of read i at position p:
 *   hashes_out[e] = h(p), pos_out[e] = p, read_out[e] = i, strand_out[e] = 1 iff the reverse complement's value is numerically
 *   smaller than the forward value under KMU_FHASH_CANON_RAW / _VALUE / _INVHASH (the k-mer the hash was taken of is the reverse
 *   complement; a palindrome gets 0), and 0 under the fhash modes that do not canonicalise.  The two ntHash modes are accepted
 *   for the ordering; a non-NULL strand_out with them is KMU_E_UNSUPPORTED (the canonical ntHash does not expose its strand here).
 * Properties: w = 1 returns every k-mer.  A read that is one k-mer repeated (poly-A) returns every window start 0 .. nwin - 1 and
 *   nothing behind it -- the usual dense behaviour of a leftmost tie rule.  KMU_FHASH_CANON_INVHASH is the recommended order:
 *   under KMU_FHASH_CANON_VALUE poly-A is everyone's minimizer.  The result is a pure function of the inputs: it does not depend
 *   on the launch shape or on timing.
 * Counts and capacity: *n_out (host memory in both modes, required) is always the total number of minimizers.
 *   hashes_out == NULL is the count-only call: it writes *n_out and, if given, mini_offsets_out, and nothing else.
 *   cap < total: KMU_E_BAD_ARG with *n_out set and the outputs unspecified.  win_offsets[n_seq] of kmu_minimizer_layout (the
 *   windows of the reads) is always a sufficient cap: a caller who takes it can skip the count-only call.
 * KMU_MEM_DEVICE: every array except n_out is device memory (mini_offsets_out lives where `offsets` lives); the call synchronises
 *   the stream once to hand n_out over, also in async_device contexts.  (The per-tile counts live in a workspace that, like every
 *   workspace of the context, only grows: a call with more tiles than any call before it on this context counts a second time.)
 *   The offsets are trusted, as kmu_sketch trusts block_row_offsets.
 * KMU_MEM_HOST: the inputs go up through the context's workspace and the results come back, as in kmu_read_anchors; a read of
 *   2^32 bases or more is KMU_E_UNSUPPORTED (positions are uint32).
 * n_seq == 0: KMU_OK, *n_out = 0.  Empty reads and reads shorter than k contribute nothing.
 * KMU_E_BAD_ARG: null ctx / p / n_out, w == 0, bad mem.  KMU_E_UNSUPPORTED: w > KMU_MINIMIZER_MAX_W, KMU_INPUT_PACKED2.
 * KMU_E_BAD_ALPHABET: an amino-acid k-mer type.  A k-mer type and k that kmu_kmer_hashes refuses is refused the same way.  A
 * non-ACGT byte anywhere in a read (reads shorter than k included) is KMU_E_NON_ACGT, reported as kmu_read_anchors reports it.
 * How: one wave per tile of KMU_MINIMIZER_TILE consecutive windows of one read, tiles dealt grid-stride, so a chromosome spreads
 *   over the device as many short reads do; neither the launches nor the host synchronisations of a call depend on the number or
 *   the lengths of the reads.  DESIGN.md 3.14 has the kernel. */
#define KMU_MINIMIZER_MAX_W 256
#define KMU_MINIMIZER_TILE 1024 /* windows one workgroup takes at a time */
/* windows per read = an upper bound of its minimizers; win_offsets_out[n_seq + 1]; plain host C, no context, no device (like
 * kmu_anchor_layout).  KMU_E_BAD_ARG: null pointers, kmer_size == 0, w == 0 or > KMU_MINIMIZER_MAX_W. */
int kmu_minimizer_layout(const uint64_t *offsets, uint32_t n_seq, uint32_t kmer_size, uint32_t w, uint64_t *win_offsets_out);
int kmu_read_minimizers(kmu_ctx *ctx, const kmu_hash_params *p, const uint8_t *bases, const uint64_t *offsets, uint32_t n_seq,
                        uint32_t w,
                        uint64_t *hashes_out,       /* NULL: the count-only call */
                        uint32_t *pos_out,          /* may be NULL */
                        uint32_t *read_out,         /* may be NULL */
                        uint8_t *strand_out,        /* may be NULL */
                        uint64_t cap,
                        uint64_t *mini_offsets_out, /* n_seq + 1, lives where `offsets` lives; may be NULL */
                        uint64_t *n_out);           /* host memory in both modes; required */

/* ---- syncmers: the closed and open (k, s, t) syncmers of every read, selected on the device --------------------------
 * Read i has L bases, nk = max(0, L - k + 1) k-mers and, with 1 <= s <= k, L - s + 1 s-mers.  h(p), p in [0, nk), is exactly the
 * value kmu_kmer_hashes writes for (p->kmer_type, p->kmer_size = k, p->fhash); g(q) the one it writes for (sp->s_kmer_type,
 * sp->s, sp->s_fhash); both 64-bit, zero-extended for the u32 types.  u = k - s; m(p) = min g(q) over q in [p, p + u]: the
 * s-mers that lie inside the k-mer at p.
 * Selection: THE K-MER AT p IS SELECTED IFF g(p + t) == m(p) OR g(p + u - t) == m(p), with 0 <= t <= u / 2 (integer division).
 *   The comparison is by value, not by position: a tie anywhere does not block a k-mer whose end s-mer holds the minimum.  A
 *   k-mer is chosen by its own k bases alone -- no neighbour takes part, unlike a window minimizer.
 * Properties: t = 0 gives closed syncmers, about 2 / (u + 1) of the k-mers of random sequence; 2 t == u gives open syncmers at
 *   the middle offset, about 1 / (u + 1).  s == k selects every k-mer, and so does a read that is one base repeated.  With a
 *   canonical s_fhash and a canonical fhash the selection is strand-symmetric, ties included: the seeds of revcomp(read) are the
 *   seeds of read at the positions nk - 1 - p, with the same hashes and the strand flipped, except on palindromic k-mers, whose
 *   strand is 0 on both.  The result is a pure function of the inputs: it does not depend on the launch shape or on timing.
 * Outputs: the selected k-mers of all reads, concatenated in read order, ascending in position within a read;
 *   sync_offsets_out[i] .. sync_offsets_out[i + 1] are the entries of read i.  Entry e of read i at position p:
 *   hashes_out[e] = h(p), pos_out[e] = p, read_out[e] = i and strand_out[e] as in kmu_read_minimizers: 1 iff the reverse
 *   complement's value is numerically smaller than the forward value under KMU_FHASH_CANON_RAW / _VALUE / _INVHASH, else 0.
 * Counts and capacity: *n_out (host memory in both modes, required) is always the total.  hashes_out == NULL is the count-only
 *   call: it writes *n_out and, if given, sync_offsets_out, and nothing else.  cap < total: KMU_E_BAD_ARG with *n_out set and the
 *   outputs unspecified.  The number of k-mers, kmu_minimizer_layout(offsets, n_seq, k, 1)[n_seq], is always a sufficient cap.
 * KMU_MEM_DEVICE: every array except n_out is device memory; the call synchronises the stream once to hand n_out over (a call
 *   with more tiles than the context's workspace holds counts a second time, as kmu_read_minimizers does).  The offsets are
 *   trusted.  KMU_MEM_HOST: the inputs go up through the workspace and the results come back; a read of 2^32 bases or more is
 *   KMU_E_UNSUPPORTED (positions are uint32).
 * n_seq == 0: KMU_OK, *n_out = 0.  Empty reads and reads shorter than k contribute nothing.
 * KMU_E_BAD_ARG: null ctx / p / sp / n_out, s == 0, s > k, t > (k - s) / 2, bad mem.  KMU_E_UNSUPPORTED: KMU_INPUT_PACKED2, or
 * a non-NULL strand_out when p->fhash is an ntHash mode (the ntHash modes are fine for s_fhash, which only orders).
 * KMU_E_BAD_ALPHABET: either type is an amino-acid type.  A (type, size) pair that kmu_kmer_hashes refuses is refused the same
 * way, for k and for s.  A non-ACGT byte anywhere in a read (reads shorter than k included) is KMU_E_NON_ACGT, reported as
 * kmu_read_minimizers reports it.
 * How: one wave per tile of KMU_SYNCMER_TILE consecutive k-mer positions of one read, tiles dealt grid-stride; a tile needs
 *   nothing of its neighbours but u more s-mers behind it.  Neither the launches nor the one synchronisation of a call depend on
 *   the number or the lengths of the reads.  DESIGN.md 3.29 has the kernel. */
typedef struct kmu_syncmer_params {
    int32_t s_kmer_type; /* the k-mer type the s-mers are hashed as */
    int32_t s;           /* 1 .. k */
    int32_t s_fhash;     /* the order of the s-mers */
    uint32_t t;          /* 0 .. (k - s) / 2 */
} kmu_syncmer_params;
#define KMU_SYNCMER_TILE 1024 /* k-mer positions one wave takes at a time */
int kmu_read_syncmers(kmu_ctx *ctx, const kmu_hash_params *p, const kmu_syncmer_params *sp, const uint8_t *bases,
                      const uint64_t *offsets, uint32_t n_seq,
                      uint64_t *hashes_out,       /* NULL: the count-only call */
                      uint32_t *pos_out,          /* may be NULL */
                      uint32_t *read_out,         /* may be NULL */
                      uint8_t *strand_out,        /* may be NULL */
                      uint64_t cap,
                      uint64_t *sync_offsets_out, /* n_seq + 1, lives where `offsets` lives; may be NULL */
                      uint64_t *n_out);           /* host memory in both modes; required */

/* ---- seed chaining: from minimizer hits to one colinear chain per read pair, at base resolution ----------------------
 * pairs[2p..] = (ea, eb): an entry of the query minimizers and an entry of the database minimizers, as kmu_anchor_index_match
 *   writes them for rows of one hash (minimizer.seed_pairs), in ANY order.  pos_* / read_* / strand_* are the arrays of
 *   kmu_read_minimizers (n_q / n_db entries, reads below n_reads_q / n_reads_db); a NULL strand array is all 0; the q arrays and the
 *   db arrays may be the same arrays (a self-join).
 * Anchors and groups: the pair (ea, eb) is an anchor of the read pair (A, B) = (read_q[ea], read_db[eb]) with relative strand
 *   s = strand_q[ea] ^ strand_db[eb], x = pos_q[ea] and y = pos_db[eb] for s = 0, y = -pos_db[eb] for s = 1 (the opposite strand is
 *   colinear when b runs backwards).  A GROUP is the set of anchors of one (A, B, s); inside it the anchors are ordered by (x, y)
 *   and i indexes that order.  Anchors equal in every field are interchangeable: no result depends on how a sort places them.
 * Score: integer arithmetic only, exact, nothing clamped before the record.  For j < i of a group, dx = x_i - x_j, dy = y_i - y_j.
 *   j is a PREDECESSOR of i iff i - KMU_CHAIN_LOOKBACK <= j, 0 < dx <= max_gap, 0 < dy <= max_gap and g = |dx - dy| <= band.  Then
 *   t(j, i) = f(j) + min(dx, dy, span) - cost(g), cost(0) = 0, cost(g) = ((g * span) >> 7) + (floor(log2 g) >> 1) for g > 0, and
 *   f(i) = max(span, max over the predecessors of t(j, i)).
 *   An anchor starts a chain of its own unless some t(j, i) is STRICTLY larger than span; among the predecessors with the same
 *   largest t the LARGEST j (the nearest) is chosen.  start(i) = start(j) and n(i) = n(j) + 1 of the chosen predecessor, otherwise
 *   start(i) = i and n(i) = 1.
 * Winner: per read pair the anchor e with the largest f over both of its groups; ties go to s = 0 before s = 1, then to the
 *   smallest i.  With b = start(e): score = min(f(e), 2^32 - 1), n_seeds = n(e), n_anchors = the size of e's group,
 *   a_start = x_b, a_end = x_e + span; s = 0: b_start = pos_db(b), b_end = pos_db(e) + span; s = 1: b_start = pos_db(e),
 *   b_end = pos_db(b) + span.
 * Reported: the winner of a read pair iff score >= min_score, n_seeds >= min_seeds and, under KMU_CHAIN_UPPER, read_a < read_b.
 *   The filters see the winner only: no runner-up takes its place, and there is one chain per read pair (no secondary chains).
 *   Order: read_a ascending, then read_b.  A pure function of the inputs: the order of the pairs, the launch shape and timing
 *   change nothing.
 * *n_out (host memory in both modes) is always the total.  out == NULL: the count-only call.  cap < total: KMU_E_BAD_ARG with
 *   *n_out set.  n_pairs == 0: KMU_OK, *n_out = 0.  KMU_MEM_DEVICE: every array except p and n_out is device memory and the call
 *   synchronises the stream once, to hand n_out over.  KMU_MEM_HOST: the arrays go up through the context's workspace and the
 *   records come back.
 * max_pos: 0, or a promise that no position is above it -- the sort then skips the passes of bytes no key can differ in.
 * KMU_E_BAD_ARG: null ctx / pairs / pos / read / p / n_out, span == 0 or > 64, max_gap == 0, min_seeds == 0, unknown flag bits, bad
 *   mem, pairs while a side has no entries or no reads.
 * KMU_E_UNSUPPORTED: n_pairs >= 2^32; a pair that names an entry >= n_q / n_db, a read >= n_reads_q / n_reads_db, a position >= 2^31
 *   or a position above a non-zero max_pos.  The arrays are read on the device in both modes: the refusal comes at the call's one
 *   synchronisation, and no such pair is ever used as an index.
 * How: one entry per pair, sorted by (read_a, read_b, s, x, y) with two stable radix sorts; one wave per group then runs the DP
 *   with the lookback window in registers (the current and the previous 64 anchors, one per lane) and a wave arg-max per anchor;
 *   one lane per read pair picks the winner, once to count and once to write.  A group of very many anchors is one wave's
 *   sequential work, and tiny groups leave lanes idle.  DESIGN.md 3.15 has the kernels. */
#define KMU_CHAIN_LOOKBACK 64      /* predecessors an anchor looks at */
#define KMU_CHAIN_UPPER 1u         /* flags: only read pairs with read_a < read_b */
typedef struct kmu_chain_params {
    uint32_t span;       /* k of the minimizers: the bases a seed covers; 1 .. 64 */
    uint32_t max_gap;    /* largest step in either read between chained seeds, > 0 */
    uint32_t band;       /* largest |dx - dy| between chained seeds */
    uint32_t min_seeds;  /* report chains with at least this many seeds (>= 1) */
    uint32_t min_score;
    uint32_t max_pos;    /* 0, or a promise that every position is <= max_pos: lets the sort skip dead passes */
    uint32_t flags;
} kmu_chain_params;
typedef struct {         /* 40 bytes */
    uint32_t read_a, read_b, strand;   /* strand: 0 same, 1 opposite */
    uint32_t score, n_seeds, n_anchors;
    uint32_t a_start, a_end, b_start, b_end;
} kmu_chain;
int kmu_seed_chains(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs,
                    const uint32_t *pos_q, const uint32_t *read_q, const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q,
                    const uint32_t *pos_db, const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                    const kmu_chain_params *p, int mem, kmu_chain *out, uint64_t cap, uint64_t *n_out);

/* ---- seed chaining, every chain: all chains of every group, for mapping reads onto contigs or a reference -------------
 * Arguments, kmu_chain_params (the same flag bits), mem, out, cap, n_out, the count-only call and every refusal are those of
 *   kmu_seed_chains.  Anchors, groups, the predecessor relation, t(j, i), f(i) and the choice of the predecessor are word for word
 *   those of kmu_seed_chains: the lookback of KMU_CHAIN_LOOKBACK, "strictly larger than span", "the largest j of the largest t".
 *   pred(i) is the chosen predecessor of anchor i, or none.  Inside a group the pred links form a forest with pred(i) < i.
 * Chains: defined on the forest alone, so not by how it is walked.
 *   best(v): among v and every anchor whose pred path reaches v, the anchor d with the largest f(d); ties go to the smallest d.
 *   Every anchor e with best(e) = e is the END of one chain; its members are { v : best(v) = e }, a path of pred links that ends in
 *   e.  b is its member of smallest index and p = pred(b) where there is one (then best(p) != e: the chain branches off another).
 *   This is the decomposition that back-tracking gives when it takes the ends by descending f (then ascending index) and walks
 *   back until it meets an anchor already used (minimap2's), stated without an order of processing.
 * Record: read_a, read_b, strand of the group; n_anchors = the size of the group; n_seeds = the number of members;
 *   score = f(e) - f(p), or f(e) without a p, computed in 64 bits and clamped to 0 .. 2^32 - 1 (a branch may end below the f of the
 *   anchor it left: its score is 0); a_start, a_end, b_start, b_end from b and e by the rules of kmu_seed_chains.
 * Reported: a chain iff its clamped score >= min_score, n_seeds >= min_seeds and, under KMU_CHAIN_UPPER, read_a < read_b.  The
 *   filters act per chain: one that fails is left out, and its anchors go to no other chain.
 * Order: read_a, read_b, strand, then e, all ascending.  A pure function of the inputs.  Anchors equal in every field are
 *   interchangeable: they stand next to each other in the (x, y) order, and f, pred, best and every field of a record are
 *   functions of the sequence of (x, y) values and of positions in it -- exchanging two equal entries leaves that sequence, and so
 *   every record, as it is; which pair of the input an anchor came from is in no record.
 * Against kmu_seed_chains: every ancestor of a group's arg-max (the largest f, then the smallest index) carries it as its best, so
 *   its chain runs back to a root, has score f(e) unclamped and is the one kmu_seed_chains walks.  Among the unfiltered chains of a
 *   read pair, the first by (largest unclamped score, strand 0 before 1, smallest e) is exactly the record of kmu_seed_chains.
 * Who takes which: kmu_chain_align, kmu_chain_cigar, kmu_chain_pileup and the PAF writer take these records as they take any
 *   kmu_chain.  A pileup over several chains of one read pair counts the columns where they overlap once per chain.
 *   kmu_sg_classify, kmu_sg_graph and kmu_sg_unitig_chains keep taking the one-per-pair records of kmu_seed_chains.
 * How: keys, sorts and groups as in kmu_seed_chains; the DP also leaves f and pred per sorted anchor (12 bytes); one wave per
 *   group then sweeps the group's chunks of 64 twice with both chunks a link can span in registers: from the last anchor to the
 *   first, handing every anchor's best to the lane of its predecessor (readlane, no reduction), and from the first to the last
 *   for the count and first member of every chain; the ends that pass the filters are counted per group, the offsets scanned,
 *   and a second wave per group writes them.  No LDS, no atomics, no floating point.  DESIGN.md 3.28 has the kernels. */
int kmu_seed_chains_all(kmu_ctx *ctx, const uint32_t *pairs, uint64_t n_pairs,
                        const uint32_t *pos_q, const uint32_t *read_q, const uint8_t *strand_q, uint32_t n_q, uint32_t n_reads_q,
                        const uint32_t *pos_db, const uint32_t *read_db, const uint8_t *strand_db, uint32_t n_db, uint32_t n_reads_db,
                        const kmu_chain_params *p, int mem, kmu_chain *out, uint64_t cap, uint64_t *n_out);

/* ---- chain ranking: primary and secondary chains of every query read -------------------------------------------------
 * Input: chains[n_chains] of either chaining entry; the records of one read_a must be consecutive, with read_a non-decreasing
 *   (both entries write them so).  n_reads_q: the reads of the q batch.  out[c] belongs to chains[c]: always n_chains records, so
 *   the arrays of kmu_chain_align, kmu_chain_cigar and the rest stay aligned.
 * Inside one query read:
 *   rank: the 0-based position of the chain by score descending, then input index ascending.
 *   len = a_end - a_start; ov(c, P) = max(0, min(a_end_c, a_end_P) - max(a_start_c, a_start_P)).
 *   In rank order, chain c is SECONDARY TO an earlier primary P iff ov > 0 and ov * 1000 >= mask_permille * min(len_c, len_P)
 *   (64-bit products).  parent(c) is the input index of the best-ranked such P.  A chain with no such P is PRIMARY and
 *   parent(c) = c; a secondary is never a parent.
 *   For a primary, sub_score is the largest score of its secondaries (0 without any) and n_sub their number; for a secondary
 *   both are 0.  Integer compares only: a pure function of the input.
 * KMU_MEM_DEVICE: chains and out are device memory; the call synchronises the stream once, to read the refusal flag.
 *   KMU_MEM_HOST: the records go up through the context's workspace and the output comes back.
 * n_chains == 0: KMU_OK.  KMU_E_BAD_ARG (nothing is launched): null ctx / chains / p / out, mask_permille > 1000, non-zero flags,
 *   bad mem, chains while n_reads_q == 0.
 * KMU_E_UNSUPPORTED: n_chains >= 2^32; read_a falling from one record to the next, read_a >= n_reads_q, a_start > a_end.  These are
 *   found on the device and reported at the call's one synchronisation; no such record is used as an index, and the records of a
 *   refused call are unspecified.
 * How: one key per chain, (read_a, ~score) with the index as value, sorted by the stable radix sort (only the bytes n_reads_q
 *   reaches, and the four of the score); the first sorted chain of every read by binary search; one wave per query read walks
 *   its chains in rank order with the primaries so far in its lanes, tests a chain against them 64 at a time, and a ballot finds
 *   the first hit.  A read of c chains costs up to c^2 / 64 such tests in one wave: the accepted limit -- reads have tens of
 *   chains, not tens of thousands.  DESIGN.md 3.28 has the kernels. */
typedef struct kmu_rank_params {
    uint32_t mask_permille;  /* 0 .. 1000: the share of the shorter chain's query interval that must be covered */
    uint32_t flags;          /* no flag bits yet: must be 0 */
} kmu_rank_params;
typedef struct { uint32_t rank, parent, sub_score, n_sub; } kmu_chain_rank_rec;   /* 16 bytes */
int kmu_chain_rank(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, uint32_t n_reads_q,
                   const kmu_rank_params *p, int mem, kmu_chain_rank_rec *out);

/* ---- chain alignment: banded edit distance and matches of the two segments a chain names -----------------------------
 * Segments: record c names A = read `read_a` of the q batch, bases [a_start, a_end), and B = read `read_b` of the db batch, bases
 *   [b_start, b_end); bases_* / offsets_* are KMU_INPUT_ASCII batches (letters of ACGTacgt, case does not matter) of n_reads_q /
 *   n_reads_db reads.  For strand == 1 B is replaced by its reverse complement; the b coordinates stay forward coordinates of read
 *   b, which is what kmu_seed_chains writes.  The q arrays and the db arrays may be the same arrays (a self-join).  m = |A|,
 *   n = |B|; either may be 0.
 * Band: cell (i, j), 0 <= i <= m, 0 <= j <= n, is inside the band iff lo <= j - i <= hi with lo = min(0, n - m) - band and
 *   hi = max(0, n - m) + band; n_diags = hi - lo + 1 = |n - m| + 2 band + 1.  Both corners are always inside.
 * Value: global alignment with unit costs.  The value of a cell is the lexicographic minimum of (edits, -matches) over all paths
 *   from (0, 0) that stay inside the band: a diagonal step over equal bases adds (0, -1); a diagonal step over different bases, a
 *   horizontal and a vertical step add (1, 0) each.  edit and matches are those of cell (m, n).  The value is unique: a pure
 *   function of the inputs -- the launch shape and timing change nothing, and no tie rule between moves is needed.  The length of
 *   the alignment block (PAF column 11) is matches + edit.
 * Flags: KMU_ALN_DONE iff n_diags <= KMU_ALIGN_MAX_DIAGS; otherwise the record is {UINT32_MAX, 0, n_diags, 0}, the chain does no
 *   work and its bases are not looked at.  KMU_ALN_EXACT iff DONE and edit - |n - m| <= 2 band: a path with d edits leaves the
 *   diagonals between 0 and n - m by at most (d - |n - m|) / 2, so every optimal path of the unbanded problem then lies inside the
 *   band and both fields are the unbanded ones.
 * Output: out[c] belongs to chains[c]; always n_chains records -- no count call, no capacity.
 * KMU_MEM_DEVICE: every array except p is device memory (offsets_* live with the bases); the call synchronises the stream once, to
 *   read the refusal flags, also in async_device contexts.  KMU_MEM_HOST: the arrays go up through the context's workspace and the
 *   records come back, as in kmu_seed_chains.
 * n_chains == 0: KMU_OK.  KMU_E_BAD_ARG (nothing is launched): null ctx / chains / bases / offsets / p / out, non-zero flags,
 *   2 band + 1 > KMU_ALIGN_MAX_DIAGS, bad mem, chains while a side has no reads.
 * KMU_E_UNSUPPORTED: a record with a read >= n_reads_q / n_reads_db, strand > 1, a start above its end or an end above the length
 *   of its read.  KMU_E_NON_ACGT: a byte outside ACGTacgt inside an aligned segment (a segment of a chain without DONE is not
 *   aligned).  Both are found on the device and reported at the call's one synchronisation (UNSUPPORTED first); no such record is
 *   ever used as an index, and the records of a refused call are unspecified.
 * How: one wave per chain, chains dealt grid-stride.  The band lives in the lanes -- a lane owns 1, 2, 4 or 8 pairs of adjacent
 *   diagonals, by the chain's n_diags -- and the wave sweeps the anti-diagonals two at a time with one 64-bit value per diagonal in
 *   registers and the neighbours' values by DPP wave shifts.  The bases of both segments pass through LDS as 2-bit codes,
 *   KMU_ALIGN_CHUNK bases of progress at a time; a lane shifts its next 32 of each through a register.  A chain is m + n + 1
 *   sequential anti-diagonals of one wave: a 50 kb overlap is 100 k steps, which is the accepted limit.  DESIGN.md 3.16 has the
 *   kernel. */
#define KMU_ALIGN_MAX_DIAGS 1024   /* the widest band, in diagonals, one chain may need */
#define KMU_ALIGN_CHUNK 512        /* bases of progress along either segment between two stagings of the kernel */
#define KMU_ALN_DONE  1u           /* the segment pair was aligned */
#define KMU_ALN_EXACT 2u           /* edit and matches are those of the unbanded problem */
typedef struct kmu_align_params {
    uint32_t band;
    uint32_t flags;      /* no flag bits yet: must be 0 */
} kmu_align_params;
typedef struct {         /* 16 bytes */
    uint32_t edit, matches, n_diags, flags;
} kmu_chain_aln;
int kmu_chain_align(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains,
                    const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                    const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db,
                    const kmu_align_params *p, int mem, kmu_chain_aln *out);

/* ---- chain alignment paths: the CIGAR of every chain, traced on the device ---------------------------------------------
 * Segments, band, cell values, KMU_ALN_DONE, KMU_ALN_EXACT and the refusals are exactly those of kmu_chain_align: aln_out[c] is
 *   the record kmu_chain_align writes for chains[c] at the same band, plus KMU_ALN_PATH, set iff the chain's runs were written.
 * Path: defined on the cell values only, backwards from (m, n), so it is a pure function of the inputs like the values are.  At
 *   (0, 0) the walk stops; at i = 0 the step is left, at j = 0 it is up; elsewhere the first of these that applies:
 *   diagonal, to (i - 1, j - 1), if v(i - 1, j - 1) plus the cost of that step equals v(i, j); otherwise up, to (i - 1, j), if
 *   v(i - 1, j) plus one edit equals v(i, j); otherwise left, to (i, j - 1).  A diagonal over equal bases is `=`, over different
 *   bases `X`; up consumes a base of A (the query) only and is `I`; left consumes a base of B' only and is `D`.  A = AA against
 *   B = A at any band >= 1 is 1I1=, not 1=1I.
 * Output: the runs of a chain in path order from (0, 0) to (m, n) -- A forward against B, or against the reverse complement of B
 *   for strand 1 -- each one uint32, len << 4 | op with BAM's codes (KMU_CIGAR_*).  Adjacent runs have different ops, except that
 *   a run longer than KMU_CIGAR_MAX_RUN is cut: the remainder comes first, every later piece is KMU_CIGAR_MAX_RUN long.  The runs
 *   of chain c are ops_out[op_offsets_out[c] .. op_offsets_out[c + 1]); op_offsets_out has n_chains + 1 entries and lives where
 *   the other arrays live.  A chain without PATH has no runs.  For a chain with PATH: sum(=) = matches, sum(X) + sum(I) + sum(D)
 *   = edit, sum(=) + sum(X) + sum(I) = m, sum(=) + sum(X) + sum(D) = n; m = n = 0 has PATH and no runs.
 * Counting and capacity: *n_ops_out (host memory in both modes) is always the total.  ops_out == NULL: the count-only call --
 *   aln_out and op_offsets_out are written all the same.  cap < total: KMU_E_BAD_ARG with *n_ops_out set; nothing is written
 *   beyond cap.  A chain has at most 2 edit + 1 runs (every run that is not `=` holds an edit; pieces of cut runs come on top),
 *   so a caller who holds the kmu_chain_aln records of the same band can size ops_out without a count call.
 * Trace memory: the walk reads two bits per cell that the sweep wrote down: ceil(steps C / 8) * 256 bytes for a chain with
 *   DONE, steps = (m + n) / 2 + 1 or + 2 and C = 1, 2, 4, 8 for n_diags up to 128, 256, 512, 1024.  The bits of a batch of chains
 *   live in the context's workspace, and the call never asks the workspace for more than max_trace_bytes of them (the workspace
 *   rounds a request up by an eighth): it cuts the chains, in their order, into consecutive batches that fit.  No result depends
 *   on the budget, with one exception: a chain whose own trace is above it is aligned as kmu_chain_align aligns it -- edit,
 *   matches, DONE, EXACT -- and has no PATH and no runs.  Budgets above 2^40 - 256 bytes are that.
 * KMU_MEM_DEVICE: every array except p and n_ops_out is device memory.  The call synchronises the stream twice whatever the number
 *   of batches: once for the plan (the refusal of bad records comes here, before any alignment) and once at the end; KMU_MEM_HOST
 *   a third time, to bring down the runs once their number is known.
 * n_chains == 0: KMU_OK, *n_ops_out = 0, op_offsets_out[0] = 0.  KMU_E_BAD_ARG (nothing is launched): null ctx / chains / bases /
 *   offsets / p / aln_out / op_offsets_out / n_ops_out, non-zero flags, 2 band + 1 > KMU_ALIGN_MAX_DIAGS, bad mem, chains while a
 *   side has no reads.
 * KMU_E_UNSUPPORTED: a record with a read >= n_reads_q / n_reads_db, strand > 1, a start above its end or an end above the length
 *   of its read.  KMU_E_NON_ACGT: a byte outside ACGTacgt inside an aligned segment (a segment of a chain without DONE is not
 *   aligned).  Both are found on the device and reported at a synchronisation (UNSUPPORTED first); no such record is ever used
 *   as an index, and the outputs of a refused call are unspecified.
 * How: the sweep of kmu_chain_align with one more duty: a lane packs the two bits of its cells of 8 / C pair-steps into a word
 *   and the wave stores the word of all lanes as one 256-byte row; nothing in the sweep waits for these stores.  A second kernel
 *   walks back, one wave per chain, over rows it stages in LDS 32 at a time, and writes the runs into the end of the chain's own
 *   slab; a scan of the run counts and a copy put them in place.  One wave per chain in both; the walk is one lane's work.
 *   DESIGN.md 3.17 has the kernels. */
#define KMU_ALN_PATH  4u           /* kmu_chain_cigar: the chain's runs were written */
#define KMU_CIGAR_I 1u             /* BAM's codes: a base of A only */
#define KMU_CIGAR_D 2u             /* a base of B' only */
#define KMU_CIGAR_EQ 7u            /* a column of equal bases */
#define KMU_CIGAR_X 8u             /* a column of different bases */
#define KMU_CIGAR_MAX_RUN 268435455u /* 2^28 - 1: the longest run one uint32 holds */
/* 8 GiB.  The workload the project measures with (20 000 ONT-shaped reads, 34 085 chains, 8.0e7 pair-steps) runs at C = 2 for
 * band 64 (n_diags >= 129): 64 bytes a pair-step, 5.12 GB measured -- one batch with room to spare; band 256 (C = 8, 256 bytes a
 * pair-step, 20.47 GB measured) is three batches.  Every batch ends with the tail of its longest chains, so a caller with the
 * memory to spare at wide bands gains from a larger budget (DESIGN.md 3.17 has the figures).  An MI355X has 288 GB; 8 GiB
 * leaves the rest to the caller's own arrays. */
#define KMU_CIGAR_TRACE_DEFAULT 8589934592ull
typedef struct kmu_cigar_params {
    uint32_t band;
    uint32_t flags;             /* must be 0 */
    uint64_t max_trace_bytes;   /* 0 = KMU_CIGAR_TRACE_DEFAULT */
} kmu_cigar_params;
int kmu_chain_cigar(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains,
                    const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                    const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db,
                    const kmu_cigar_params *p, int mem,
                    kmu_chain_aln *aln_out, uint64_t *op_offsets_out,
                    uint32_t *ops_out, uint64_t cap, uint64_t *n_ops_out);

/* ---- read pileup: per-base votes of every chain's runs onto both reads ---------------------------------------------------
 * Inputs: the inputs and the outputs of ONE kmu_chain_cigar call -- chains, aln (its records), op_offsets (n_chains + 1), ops, n_ops
 *   (the total) -- and the two KMU_INPUT_ASCII batches; the db arrays may be the q arrays (a self-join).
 * Tables: pile_q / pile_db have one row per base of their batch; row offsets[read] + pos is KMU_PILE_COLS uint32 (32 bytes) indexed
 *   by KMU_PILE_*.  The call ADDS to what the tables hold: the caller zeroes them, and several calls (several db batches against
 *   one q batch) accumulate.  pile_q and pile_db may be the same array when the two batches are the same arrays -- the self-join
 *   under KMU_CHAIN_UPPER, where every read then collects the votes of all its partners.
 * flags: KMU_PILE_Q votes onto the A side, KMU_PILE_DB onto the B side; at least one; the table of a side not asked for may be NULL.
 * Which chains vote: those whose aln record has KMU_ALN_PATH.  Every other chain must have no runs and votes nothing.
 * Coordinates: the runs of a chain follow A forwards against B' (B on strand 0, its reverse complement on strand 1) from
 *   (i, j) = (0, 0): `=` and `X` advance both and are treated alike, as a diagonal column -- no bases are compared; `I` advances i,
 *   `D` advances j.  Base i of A is row offsets_q[read_a] + a_start + i; base j of B' is base b_start + j of read b on strand 0 and
 *   b_end - 1 - j on strand 1.
 * A side: a diagonal column (i, j) adds 1 to the letter of B' at j (on strand 1 the complement of B's forward letter) in A's row i;
 *   each base i of an I run adds 1 to DEL in row i; a D run of length L lies between A's bases i - 1 and i and adds 1 to INS and L
 *   to INS_BASES in row i - 1, nothing for i = 0.
 * B side, in forward coordinates and forward letters of read b: a diagonal column adds 1 to A's letter at i (complemented on
 *   strand 1) in B's row for j; each base of a D run adds 1 to DEL; an I run of length L adds 1 to INS and L to INS_BASES in the row
 *   of the base before the gap in read b's forward direction: B' index j - 1 on strand 0 (nothing for j = 0), B' index j on strand 1
 *   (nothing for j = n).
 * ENDS: on each side asked for, a voting chain with a non-empty segment adds 1 at the first row of its segment and 1 at the last (a
 *   segment of one base gets 2).
 * It follows: for one voting chain alone A + C + G + T + DEL is 1 on every row of its segment and 0 elsewhere, on both sides; the
 *   counts are sums of integers, so the order of the chains, the launch shape and timing change nothing; a cut run votes as the two
 *   runs it is (two INS).
 * KMU_MEM_DEVICE: every array except p is device memory; the call synchronises the stream twice: after the checks and at the end.
 *   KMU_MEM_HOST: the arrays go up through the context's workspace and the votes come back added to the caller's tables.
 * n_chains == 0: KMU_OK.  KMU_E_BAD_ARG (nothing is launched): null ctx / chains / aln / op_offsets / bases / offsets / p, ops null
 *   with n_ops > 0, flags 0 or with unknown bits, a null table for a side asked for, one table for both sides of two different
 *   batches, bad mem, chains while a side has no reads.
 * KMU_E_UNSUPPORTED, found on the device BEFORE any vote -- a refused call leaves both tables untouched: a record kmu_chain_cigar
 *   would refuse; op_offsets that decrease or end above n_ops; runs on a chain without PATH; a run with an op outside {I, D, =, X} or
 *   of length 0; a PATH chain whose runs do not sum to m on A and to n on B.  No inconsistent run is ever used as an index.
 * KMU_E_NON_ACGT: a voted letter outside ACGTacgt (a letter of a side that is not voted is not looked at); the tables are then
 *   unspecified.
 * How: the runs of every chain are cut into tiles of 64.  One wave per chain sums the bases its tiles consume -- the checks, and
 *   (i, j) at the start of every tile; a scan gives the tile offsets.  The vote kernel takes one wave per tile: it scans the tile's
 *   column counts and walks the columns 64 at a time, one column per lane, so a wave's atomic adds (plain uint32) fall on about 64
 *   consecutive rows; a run's INS votes come from the lane that owns the run.  A long chain spreads over as many waves as it has
 *   tiles.  DESIGN.md 3.18 has the kernels. */
#define KMU_PILE_COLS 8            /* uint32 per row */
#define KMU_PILE_A 0               /* votes for a letter: A, C, G, T */
#define KMU_PILE_C 1
#define KMU_PILE_G 2
#define KMU_PILE_T 3
#define KMU_PILE_DEL 4             /* partners aligned over the base that have nothing there */
#define KMU_PILE_INS 5             /* partners with extra bases behind the base */
#define KMU_PILE_INS_BASES 6       /* ... and how many bases in all */
#define KMU_PILE_ENDS 7            /* segments that begin or end at the base */
#define KMU_PILE_Q 1u              /* flags: vote onto the A side */
#define KMU_PILE_DB 2u             /* vote onto the B side */
typedef struct kmu_pileup_params {
    uint32_t flags;
} kmu_pileup_params;
int kmu_chain_pileup(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln,
                     const uint64_t *op_offsets, const uint32_t *ops, uint64_t n_ops,
                     const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                     const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db,
                     const kmu_pileup_params *p, int mem, uint32_t *pile_q, uint32_t *pile_db);

/* ---- pileup calls: a call per base and a summary per read from a table of kmu_chain_pileup ------------------------------
 * pile: the table of the batch (bases, offsets, n_reads).  Per base g, depth = A + C + G + T + DEL.
 * call_out[g] (n_bases bytes; may be NULL): bits 0..2 are KMU_CALL_NONE if depth < min_depth, otherwise the code 0..4 (KMU_PILE_A ..
 *   KMU_PILE_DEL) with the largest count; ties go to the read's own base if it is among the tied codes, otherwise to the smallest
 *   code; a read base outside ACGTacgt equals no code.  KMU_CALL_INS: called and 2 INS > depth.  KMU_CALL_DIFF: called and the
 *   code differs from the read's own base (a DEL call always differs).
 * reads_out[r] (n_reads records; may be NULL, not both): the summary of read r; its counts are of rows with depth >= min_depth.
 * min_depth >= 1; flags must be 0.  n_reads == 0: KMU_OK.  KMU_E_BAD_ARG: null ctx / pile / bases / offsets / p, both outputs null,
 *   min_depth == 0, non-zero flags, bad mem.  KMU_MEM_DEVICE: every array except p is device memory; KMU_MEM_HOST: through the
 *   workspace.  The pileup counts insertions; kmu_pile_ins_plan and kmu_chain_pile_ins below collect the inserted letters, and
 *   kmu_pile_consensus writes the corrected reads.
 * How: one lane per base for the calls; one wave per read, 64 rows at a time, for the summaries. */
#define KMU_CALL_NONE 7u           /* bits 0..2: the depth is below min_depth */
#define KMU_CALL_INS 8u            /* most partners have extra bases behind this one */
#define KMU_CALL_DIFF 16u          /* the call is not the read's own base */
typedef struct kmu_pile_call_params {
    uint32_t min_depth;  /* >= 1 */
    uint32_t flags;      /* must be 0 */
} kmu_pile_call_params;
typedef struct {         /* 32 bytes */
    uint32_t n_bases;    /* bases of the read */
    uint32_t covered;    /* rows with depth >= min_depth */
    uint32_t n_diff;     /* covered rows with KMU_CALL_DIFF */
    uint32_t n_del;      /* covered rows called KMU_PILE_DEL */
    uint32_t n_ins;      /* covered rows with KMU_CALL_INS */
    uint32_t max_depth;  /* largest depth over the read's rows (2^32 - 1 if it is above) */
    uint64_t depth_sum;  /* sum of depth over all rows of the read */
} kmu_read_pile;
int kmu_pile_call(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                  const kmu_pile_call_params *p, int mem, uint8_t *call_out, kmu_read_pile *reads_out);

/* ---- read correction: the inserted letters, and the consensus sequence of every read -------------------------------------
 * Three calls close the pipeline reads -> chains -> runs -> pileup -> calls on the device.  kmu_pile_ins_plan gives every base a
 * number of insertion SLOTS, kmu_chain_pile_ins votes the letters of every chain's gap runs into them, and kmu_pile_consensus writes
 * the corrected reads as a new KMU_INPUT_ASCII batch.
 *
 * kmu_pile_ins_plan.  pile and call: the table of one batch as kmu_chain_pileup left it and the call bytes kmu_pile_call made from
 *   it; n_bases rows.  ins_len_out[g] (n_bases bytes) is the slot count of row g: 0 unless call[g] has KMU_CALL_INS; otherwise
 *   min(max_ins, floor((2 INS_BASES - 1) / depth)) with depth = A + C + G + T + DEL, computed in 64 bits (0 where depth or INS_BASES
 *   is 0, which no call byte made from the table allows).  That is the largest number k of inserted positions at which more than
 *   half of the depth can still have a letter: the partners with at least k inserted bases number at most INS_BASES / k.  It is at
 *   least 1 on every row with KMU_CALL_INS, since 2 INS_BASES >= 2 INS > depth.  *n_slots_out (host memory in both modes) is the sum.
 *   Slot index: slot s of row g has the global index S(g) + s, S being the exclusive prefix sum of ins_len over the batch's rows;
 *   this is public contract.  The two calls below recompute what they need of S from ins_len alone: a caller holds only the bytes.
 *   n_bases == 0: KMU_OK, *n_slots_out = 0.  KMU_E_BAD_ARG: null ctx / pile / call / p / ins_len_out / n_slots_out, max_ins 0 or above
 *   KMU_INS_MAX, non-zero flags, bad mem.
 *
 * kmu_chain_pile_ins.  Inputs, flags (KMU_PILE_Q, KMU_PILE_DB), coordinates and the chains that vote are exactly those of
 *   kmu_chain_pileup.  ins_len_q / ins_len_db and n_slots_q / n_slots_db: the plan of each voted batch.  ins_q / ins_db: uint32
 *   [n_slots][KMU_INS_COLS], one count per letter A C G T of every slot; the call ADDS to them.  ins_q and ins_db may be the same
 *   array when the two batches are the same arrays (then ins_len and n_slots must be the same too), as in the pileup; what belongs to
 *   a side not asked for may be NULL / 0.
 *   A side: a D run of length L that begins at (i0, j0) with i0 >= 1 has the row g = offsets_q[read_a] + a_start + i0 - 1; for
 *   k < min(L, ins_len[g]) it adds 1 in slot S(g) + k to the letter of B' at j0 + k (on strand 1 the complement of B's forward letter).
 *   B side: an I run of length L that begins at (i0, j0) has the row that takes its INS vote in kmu_chain_pileup -- B' index j0 - 1 on
 *   strand 0, j0 on strand 1, none at the segment's edge -- and its slots run in read b's forward direction: on strand 0 slot k takes
 *   A's letter at i0 + k, on strand 1 the complement of A's letter at i0 + L - 1 - k.
 *   A cut run and two adjacent runs of one op vote as the separate runs they are, each from slot 0.  Letters beyond a row's slots are
 *   dropped.  Integer sums only: the order of the chains, the launch shape and timing change nothing.
 *   KMU_MEM_DEVICE: every array except p is device memory; the call synchronises the stream four times (the checks of the runs, the
 *   sizes of the two batches, the check of ins_len, the end).  KMU_MEM_HOST: through the workspace; the votes come back added to the caller's tables.
 *   n_chains == 0: KMU_OK, nothing is looked at.  KMU_E_BAD_ARG: what kmu_chain_pileup refuses so (the tables being ins_q / ins_db), a
 *   null ins_len of a side asked for, one table for both sides with two ins_len or two n_slots.
 *   Found on the device BEFORE any vote, the tables untouched: KMU_E_UNSUPPORTED for everything kmu_chain_pileup refuses so, and where
 *   the sum of a voted side's ins_len is not its n_slots.  No inconsistent run or ins_len is ever used as an index.
 *   KMU_E_NON_ACGT: a voted letter outside ACGTacgt; the tables are then unspecified.
 *   How: the check and tile step of kmu_chain_pileup, the same code.  One wave per tile of 64 runs, one run per lane; only a lane that
 *   owns a gap run of a voted side loads the byte ins_len[g], and only where that is not 0 it looks up S(g) and does at most ins_len
 *   letter loads and atomic adds.  S(g): a workspace array holds the exclusive scan of the sums of ins_len over blocks of 64 rows (8
 *   bytes per 64 rows), and the lane adds the at most 63 bytes before g inside its block.
 *
 * kmu_pile_consensus.  pile, call, ins_len, n_slots, ins: of one batch (bases, offsets, n_reads), as the calls above left them; ins
 *   may be NULL when n_slots is 0.  The output of row g, in order: its own position -- the read's own byte, verbatim, whatever it is,
 *   where bits 0..2 of call[g] are KMU_CALL_NONE (or 5 or 6, which kmu_pile_call never writes); the letter in upper case where they
 *   are a code A .. T; nothing where they are KMU_PILE_DEL -- and then, where ins_len[g] > 0, the emitted slots k = 0, 1, ...: with n_k
 *   the sum of the slot's four counts, slot k is emitted iff 2 n_k > depth(g), and emission stops at the first slot that is not, so any
 *   table gives a defined result; the letter is the one with the largest count, the smallest code among equals.  The output of read r
 *   is that of its rows in order: cons_out[cons_offsets_out[r] .. cons_offsets_out[r + 1]); cons_offsets_out has n_reads + 1 entries
 *   and lives where the other arrays live.  A read may come out empty.
 *   Counting and capacity: *n_cons_out (host memory in both modes) is always the total.  cons_out == NULL: the count-only call -- the
 *   offsets are written all the same.  cap < total: KMU_E_BAD_ARG with *n_cons_out set and the offsets written; cons_out is not written.
 *   A row gives at most one byte and its slots: total <= n_bases + n_slots, so a caller can size cons_out without a count call.
 *   n_reads == 0: KMU_OK, one offset (0).  KMU_E_BAD_ARG: null ctx / pile / call / ins_len / bases / offsets / p / cons_offsets_out /
 *   n_cons_out, ins null with n_slots > 0, non-zero flags, bad mem.  KMU_E_UNSUPPORTED, before any output: the sum of ins_len is not
 *   n_slots.  KMU_MEM_DEVICE: every array except p and n_cons_out is device memory; KMU_MEM_HOST: through the workspace.
 *   How: tiles are 64 consecutive rows of the batch, not reads, so a chromosome-long read is many waves' work.  One wave per tile, one
 *   row per lane: three byte loads per row, the pile row and the slots only where ins_len > 0.  A count pass leaves tile sums, a scan
 *   makes tile offsets, a write pass repeats the row rule behind a wave prefix sum; one lane per read derives its offset from the tile
 *   that holds its first row.  DESIGN.md 3.19 has the kernels. */
#define KMU_INS_COLS 4             /* uint32 per slot: votes for A, C, G, T */
#define KMU_INS_MAX 255u           /* the most slots a base can get */
typedef struct kmu_ins_plan_params {
    uint32_t max_ins;    /* 1 .. KMU_INS_MAX */
    uint32_t flags;      /* must be 0 */
} kmu_ins_plan_params;
typedef struct kmu_consensus_params {
    uint32_t flags;      /* must be 0 */
} kmu_consensus_params;
int kmu_pile_ins_plan(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, uint64_t n_bases,
                      const kmu_ins_plan_params *p, int mem, uint8_t *ins_len_out, uint64_t *n_slots_out);
int kmu_chain_pile_ins(kmu_ctx *ctx, const kmu_chain *chains, uint64_t n_chains, const kmu_chain_aln *aln,
                       const uint64_t *op_offsets, const uint32_t *ops, uint64_t n_ops,
                       const uint8_t *bases_q, const uint64_t *offsets_q, uint32_t n_reads_q,
                       const uint8_t *bases_db, const uint64_t *offsets_db, uint32_t n_reads_db,
                       const kmu_pileup_params *p, int mem,
                       const uint8_t *ins_len_q, uint64_t n_slots_q, uint32_t *ins_q,
                       const uint8_t *ins_len_db, uint64_t n_slots_db, uint32_t *ins_db);
int kmu_pile_consensus(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots,
                       const uint32_t *ins, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                       const kmu_consensus_params *p, int mem,
                       uint64_t *cons_offsets_out, uint8_t *cons_out, uint64_t cap, uint64_t *n_cons_out);

/* ---- read trimming: supported segments of every read, byte ranges as a new batch, raw rows in corrected coordinates -----------
 * kmu_pile_segments.  pile: the table of one batch (offsets, n_reads) as kmu_chain_pileup left it.  Per row g,
 *   depth(g) = A + C + G + T + DEL and ends(g) = ENDS, both taken in 64 bits (A = 2^32 - 1, C = 1 is depth 2^32, not 0);
 *   good(g) <=> depth(g) >= min_depth; span(g) = max(depth(g) - ends(g), 0).
 *   Link: for two consecutive rows g - 1 and g of ONE read, link(g) holds iff both are good and
 *   max(span(g), span(g - 1)) >= min_span.  min_span == 0 links every good pair.
 *   Why: the partners that cover both g - 1 and g number exactly depth(g) - begins_at(g) = depth(g - 1) - ends_at(g - 1).  ENDS holds
 *   begins + ends, so depth - ENDS is a lower bound of that spanning depth which needs nothing but the table, and the larger of the
 *   two bounds is still one.  At a chimeric join the alignments of the left parent end at g - 1 and those of the right parent begin
 *   at g: the bound is 0 there although both rows are deep.
 *   Segment: a maximal run of rows of one read in which consecutive rows are linked; it never crosses a read boundary, even when the
 *   last row of one read and the first row of the next are both good.  Segments with end - start >= min_len are KEPT.
 *   segs_out: the kept segments in (read, start) order, [start, end) in read coordinates, rank counting the kept segments of the
 *   read from 0.  seg_offsets_out (n_reads + 1 entries): the first listed segment of every read.  With KMU_SEG_LONGEST only the
 *   longest kept segment of each read is listed, the leftmost among equals, with the rank it has among the read's kept segments.
 *   reads_out[r] does not depend on that flag.
 *   Counting and capacity: *n_segs_out (host memory in both modes) is always the number of listed segments.  segs_out == NULL: the
 *   count-only call -- offsets and summaries are written all the same.  cap < total: KMU_E_BAD_ARG with *n_segs_out set, the offsets
 *   and the summaries written; segs_out is not written.  Kept segments are disjoint and at least min_len long: total <= n_bases /
 *   min_len (and <= n_reads with KMU_SEG_LONGEST), so a caller can size segs_out without a count call.  (Two kept segments may touch
 *   -- a flush join -- so no bound divides by min_len + 1.)
 *   Either of seg_offsets_out and reads_out may be NULL, not both together with segs_out.  n_reads == 0: KMU_OK, one offset (0).
 *   KMU_E_BAD_ARG, nothing is written: null ctx / pile / offsets / p / n_segs_out, no output at all, min_depth 0, min_len 0, unknown
 *   flag bits, bad mem.  KMU_MEM_DEVICE: every array except p and n_segs_out is device memory, pile 16-byte aligned; the call
 *   synchronises the stream three times (the batch's size; the number of runs; the total) and once more behind the copy of the
 *   segments.  KMU_MEM_HOST: through the context's workspace.
 *   The result is a pure function of the input: integer compares and integer sums only; the launch shape and timing change nothing.
 *   How: a bitmap marks the first row of every read.  Tiles are 1024 consecutive rows of the batch, not reads; a wave takes a tile 64
 *   rows at a time, gets the row before each lane's by a wave shift, and compacts run starts and run ends separately by ballot and
 *   prefix count (count pass, scan, write pass); the k-th start and the k-th end are one run.  One lane per run finds its read, adds
 *   its length to the read's n_good and marks it kept; two scans place the kept runs; one lane per read makes the summary.
 *   DESIGN.md 3.20 has the kernels.
 *
 * kmu_extract_ranges.  Output read i is bases[begin[i] .. end[i]), verbatim; out_offsets has n_ranges + 1 entries.  Ranges may be
 *   empty, overlap, repeat and come in any order.  *n_out (host memory in both modes) is always the total; out == NULL: the
 *   count-only call, the offsets are written; cap < total: KMU_E_BAD_ARG with *n_out set and the offsets written, out not written.
 *   n_ranges == 0: KMU_OK, one offset (0).  KMU_E_BAD_ARG: null ctx / out_offsets / n_out, bases null with n_bases > 0, begin or end
 *   null with n_ranges > 0, bad mem.  KMU_E_UNSUPPORTED, found on the device BEFORE anything is written (out and out_offsets stay
 *   untouched): any begin[i] > end[i] or end[i] > n_bases.  No range is ever used as an address before the check.
 *   KMU_MEM_DEVICE: every array except n_out is device memory; two synchronisations (the check with the total; the end).
 *   How: tiles are 4096 OUTPUT bytes.  A wave finds the range of its tile's first byte by a 64-ary search over out_offsets that takes
 *   the largest range, so empty ranges are skipped, and walks on 64 bytes at a time: the next 64 offsets sit one per lane, and every
 *   lane finds its own range among them with six wave shuffles.  One long range spreads over many waves; thousands of one-byte ranges
 *   share one wave.  Byte loads and stores.
 *
 * kmu_pile_consensus_pos.  The inputs of kmu_pile_consensus.  pos_out[i] (n_rows entries, where the arrays live) is the number of
 *   consensus bytes that the rows before row rows[i] of the batch produce; rows[i] == n_bases gives the total.  Hence rows = offsets
 *   reproduces cons_offsets_out of kmu_pile_consensus exactly, and read r's raw position x lands at pos(offsets[r] + x) -
 *   pos(offsets[r]) of the corrected read.  n_rows == 0: KMU_OK.  KMU_E_BAD_ARG: what kmu_pile_consensus refuses so of its inputs;
 *   rows or pos_out null with n_rows > 0.  KMU_E_UNSUPPORTED, before any output: the sum of ins_len is not n_slots; any rows[i] >
 *   n_bases.  How: the count pass and the scan of kmu_pile_consensus, then one lane per query adds the at most 63 row lengths before
 *   its row inside its tile -- the device function that makes the read offsets of kmu_pile_consensus. */
#define KMU_SEG_LONGEST 1u         /* flags: list only the longest kept segment of every read */
#define KMU_TRIM_WHOLE 0u          /* cls: one kept segment equal to the whole read */
#define KMU_TRIM_ENDS 1u           /* one kept segment, shorter than the read */
#define KMU_TRIM_SPLIT 2u          /* two or more kept segments */
#define KMU_TRIM_NONE 3u           /* no kept segment; an empty read */
typedef struct kmu_pile_seg_params {
    uint32_t min_depth;  /* >= 1 */
    uint32_t min_span;   /* 0: depth only */
    uint32_t min_len;    /* >= 1 */
    uint32_t flags;      /* KMU_SEG_LONGEST or 0 */
} kmu_pile_seg_params;
typedef struct {         /* 16 bytes */
    uint32_t read;
    uint32_t start;      /* [start, end) in read coordinates */
    uint32_t end;
    uint32_t rank;       /* among the read's kept segments, from 0 */
} kmu_pile_seg;
typedef struct {         /* 32 bytes */
    uint32_t n_bases;    /* rows of the read */
    uint32_t n_good;     /* rows with depth >= min_depth */
    uint32_t n_segs;     /* kept segments */
    uint32_t kept;       /* their summed length */
    uint32_t best_start; /* the longest kept segment, the leftmost among equals; 0, 0 if none */
    uint32_t best_end;
    uint32_t inner_bad;  /* (end of the last kept - start of the first kept) - kept */
    uint32_t cls;        /* KMU_TRIM_* */
} kmu_read_trim;
int kmu_pile_segments(kmu_ctx *ctx, const uint32_t *pile, const uint64_t *offsets, uint32_t n_reads,
                      const kmu_pile_seg_params *p, int mem,
                      uint64_t *seg_offsets_out, kmu_pile_seg *segs_out, uint64_t cap, uint64_t *n_segs_out,
                      kmu_read_trim *reads_out);
int kmu_extract_ranges(kmu_ctx *ctx, const uint8_t *bases, uint64_t n_bases, const uint64_t *begin, const uint64_t *end,
                       uint64_t n_ranges, int mem, uint64_t *out_offsets, uint8_t *out, uint64_t cap, uint64_t *n_out);
int kmu_pile_consensus_pos(kmu_ctx *ctx, const uint32_t *pile, const uint8_t *call, const uint8_t *ins_len, uint64_t n_slots,
                           const uint32_t *ins, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads,
                           const kmu_consensus_params *p, int mem,
                           const uint64_t *rows, uint64_t n_rows, uint64_t *pos_out);

/* ---- string graph: overlap classes, contained reads, the bidirected overlap graph and its transitive reduction -------
 * Inputs: chains[n_chains], the records of a SELF-JOIN (kmu_seed_chains on one batch); aln[n_chains], the records kmu_chain_align
 *   or kmu_chain_cigar wrote for them, or NULL; offsets[n_reads + 1] of the batch -- only the lengths are used, no base is read.
 * Class of a record (class_out[c], one uint8), decided in this order.  la, lb: the lengths of read_a and read_b; s: the strand;
 *   (bs', be') = (b_start, b_end) for s = 0 and (lb - b_end, lb - b_start) for s = 1 (b in a's orientation); aL = a_start,
 *   aR = la - a_end, bL = bs', bR = lb - be'; hang = min(aL, bL) + min(aR, bR); maplen = max(a_end - a_start, b_end - b_start).
 *   1. KMU_SG_SKIP: read_a >= read_b.  The graph takes each unordered pair from the record with read_a < read_b; a self-overlap
 *      never counts.
 *   2. KMU_SG_SHORT: a_end - a_start < min_overlap or b_end - b_start < min_overlap.
 *   3. KMU_SG_LOWID: only with aln.  KMU_ALN_DONE is not set, or matches * 1000 < min_identity_permille * (matches + edit) (64 bits).
 *   4. KMU_SG_INTERNAL: hang > max_hang or hang * 1000 > maplen * int_permille (64 bits).
 *   5. KMU_SG_A_CONTAINED iff aL <= bL and aR <= bR; KMU_SG_B_CONTAINED iff aL >= bL and aR >= bR.  If both hold the shorter read is
 *      the contained one, read_b at equal length.
 *   6. KMU_SG_DOVETAIL otherwise.  Then aL != bL, and both arc lengths below are >= 1.
 * Reads (reads_out[r], kmu_sg_read): read r is CONTAINED iff some record has class A_CONTAINED with read_a == r or B_CONTAINED with
 *   read_b == r.  flags: KMU_SG_READ_CONTAINED; n_records: the records that name r as read_a or read_b and are not SKIP; out_fwd,
 *   out_rev: the surviving out-degrees of the vertices 2r and 2r + 1 (0 from kmu_sg_classify).
 * Vertices and arcs: vertex 2r is read r forward, 2r + 1 its reverse complement.  An arc v -> w of length len means that w
 *   continues v to the right by len bases.  A DOVETAIL record c whose two reads are both not contained makes exactly two arcs, each
 *   the other's MATE; with a = read_a, b = read_b:
 *     aL > bL:    (2a -> 2b + s, len bR - aR)           and (2b + (s ^ 1) -> 2a + 1, len aL - bL);
 *     otherwise:  (2a + 1 -> 2b + (s ^ 1), len bL - aL) and (2b + s -> 2a, len aR - bR).
 *   An arc record (kmu_sg_arc, 32 bytes) is from, to, len, ovl, rec, flags, unique, 0: ovl is the overlap length on the `from` read
 *   (a_end - a_start or b_end - b_start), rec is c.  Arcs are listed in (from, to, rec) order; arc_offsets_out[2 n_reads + 1] gives
 *   every vertex v its slice out(v).  Duplicate records make duplicate arcs, which are kept.
 * Reduction: a pure function of the arc set.  L(v) = the largest len of out(v) + fuzz (64 bits); first(w) is the arc of out(w) that
 *   is smallest under (len, to, rec).  For every arc f = v -> w and every arc g = w -> x: if len(f) + len(g) <= L(v), or len(g) < fuzz,
 *   or g = first(w), then EVERY arc v -> x of out(v) is marked.  An arc carries KMU_SG_ARC_REDUCED iff it or its mate is marked: the
 *   marks live per record.  This is Myers' rule (2005) without the skip of already eliminated w: a superset of the sequential
 *   result, equal to it on every consistent layout.
 * Unique: an arc that is not reduced has unique = 1 iff it is the only surviving (not reduced) arc of out(from) and its mate is the
 *   only surviving arc of out(to ^ 1); every other arc has unique = 0.  kmu_components over 2 n_reads nodes with stride 8,
 *   weight_at 6, min_weight 1 then groups the vertices into unitigs, each once per strand.
 * kmu_sg_classify writes n_chains classes and n_reads summaries, always; no count call.
 * kmu_sg_graph: *n_out (host memory in both modes) is always the number of arcs.  arcs_out == NULL: the count-only call, which writes
 *   *n_out and nothing else.  cap < total: KMU_E_BAD_ARG with *n_out set, no output is written.  2 * (the number of DOVETAIL
 *   records) is always a sufficient cap.  Otherwise class_out, reads_out and arc_offsets_out are written where given (each may be
 *   NULL), and the arcs.  KMU_MEM_DEVICE: every array except p and n_out is device memory; the call synchronises the stream once, to
 *   hand over n_out and the refusal flags, also in async_device contexts.  KMU_MEM_HOST: the arrays go up through the context's
 *   workspace and the results come back.
 * n_chains == 0: KMU_OK, no arcs, every summary zero, every offset 0.
 * KMU_E_BAD_ARG (nothing is launched): null ctx / offsets / p / n_out, null chains with n_chains > 0, null class_out or reads_out
 *   of kmu_sg_classify, non-zero flags, int_permille or min_identity_permille > 1000, bad mem, chains while there are no reads.
 * KMU_E_UNSUPPORTED: n_reads >= 2^31 or n_chains >= 2^31; a record (of any class) with a read >= n_reads, strand > 1, a start above
 *   its end, an end above the length of its read, or a read of 2^32 bases or more.  The records are read on the device: the refusal
 *   comes at the call's synchronisation, no such record is ever used as an index, and the outputs of a refused call are untouched.
 * The result is a pure function of the inputs: integer compares, idempotent stores and commuting integer atomics only; the order of
 *   the records matters only through rec, and the launch shape and timing change nothing.
 * How: one lane per record classifies; one wave per tile of KMU_SG_TILE records compacts the surviving dovetails by ballot and
 *   prefix count (count, scan, write) into (from << 32 | to, 2c + side); a stable radix sort over the bytes 2 n_reads can reach; one
 *   lane per arc rebuilds its record; one lane per vertex finds its slice, L(v) and first(v); one wave per arc f walks out(to) and
 *   marks; one lane per arc sets the flag and counts the degrees; one lane per arc sets unique.  DESIGN.md 3.22 has the kernels. */
#define KMU_SG_TILE 1024           /* records one wave compacts */
#define KMU_SG_SKIP        0u
#define KMU_SG_SHORT       1u
#define KMU_SG_LOWID       2u
#define KMU_SG_INTERNAL    3u
#define KMU_SG_A_CONTAINED 4u
#define KMU_SG_B_CONTAINED 5u
#define KMU_SG_DOVETAIL    6u
#define KMU_SG_READ_CONTAINED 1u   /* kmu_sg_read.flags */
#define KMU_SG_ARC_REDUCED 1u      /* kmu_sg_arc.flags */
typedef struct kmu_sg_params {
    uint32_t min_overlap;            /* on both reads */
    uint32_t max_hang;
    uint32_t int_permille;           /* <= 1000 */
    uint32_t min_identity_permille;  /* <= 1000; used only with aln */
    uint32_t fuzz;
    uint32_t flags;                  /* no flag bits yet: must be 0 */
} kmu_sg_params;
typedef struct {         /* 16 bytes */
    uint32_t flags;      /* KMU_SG_READ_CONTAINED */
    uint32_t n_records;  /* records of the read that are not SKIP */
    uint32_t out_fwd;    /* surviving arcs of vertex 2r */
    uint32_t out_rev;    /* surviving arcs of vertex 2r + 1 */
} kmu_sg_read;
typedef struct {         /* 32 bytes */
    uint32_t from, to, len, ovl, rec, flags, unique, zero;
} kmu_sg_arc;
int kmu_sg_classify(kmu_ctx *ctx, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains,
                    const uint64_t *offsets, uint32_t n_reads, const kmu_sg_params *p, int mem,
                    uint8_t *class_out, kmu_sg_read *reads_out);
int kmu_sg_graph(kmu_ctx *ctx, const kmu_chain *chains, const kmu_chain_aln *aln, uint64_t n_chains,
                 const uint64_t *offsets, uint32_t n_reads, const kmu_sg_params *p, int mem,
                 uint8_t *class_out,          /* may be NULL */
                 kmu_sg_read *reads_out,      /* may be NULL */
                 kmu_sg_arc *arcs_out,        /* NULL: the count-only call */
                 uint64_t cap,
                 uint64_t *arc_offsets_out,   /* 2 n_reads + 1; may be NULL */
                 uint64_t *n_out);            /* host memory in both modes; required */

/* ---- unitig layout: the ordered reads of every unitig, their coordinates and the unitig's bases ----------------------
 * Inputs of kmu_sg_unitigs: arcs[n_arcs], arc records as kmu_sg_graph writes them, in any order; reads[n_reads], its summaries, or
 *   NULL (then no read is contained); offsets[n_reads + 1] of the batch -- only the lengths are used.  The result is a pure
 *   function of the inputs, and the order of arcs does not matter.
 * Links: only arcs with unique == 1 count.  A unique arc v -> w gives next(v) = w, prev(w) = v and in(w) = its len.  Every other
 *   arc is ignored, so a branching vertex ends a unitig.
 * Arc faults, found on the device in every unique arc; the call is refused with KMU_E_UNSUPPORTED at its one synchronisation, every
 *   output is left untouched and no faulty arc is ever used as an index: from or to >= 2 n_reads; from >> 1 == to >> 1; len above
 *   the length of the `to` read; the arc also carries KMU_SG_ARC_REDUCED; a vertex has two unique out-arcs or two unique in-arcs; a
 *   unique arc v -> w has no unique arc w^1 -> v^1 (its mate); a unique arc touches a read that reads flags as contained.
 *   With these checks the unique arcs form vertex-disjoint paths and cycles, each with a distinct twin on the other strand, and no
 *   path holds both vertices of a read.  Proof: out- and in-degree are at most 1, so the components are paths and cycles.  The
 *   mates of a path's arcs form the path of the complemented vertices backwards, its twin (two in-arcs of w would need two mates
 *   out of w^1, which the out-degree check excludes just as well).  A path from v to v^1 would be its own twin, walked backwards;
 *   its middle would be a vertex equal to its complement or an arc x -> x^1 between a read and itself, and neither exists.
 * Members: with reads, a read flagged KMU_SG_READ_CONTAINED is on no unitig and its place is {KMU_SG_NONE, 0, 0, 0}.  Every other
 *   read is on exactly one unitig; a read without a unique arc is a unitig of one read.
 * Orientation: of a path (or cycle) and its twin, the one kept is the one whose smallest vertex id is even: the strand on which the
 *   unitig's smallest read is forward.
 * Order: a kept path runs from its vertex without prev to its vertex without next.  A kept cycle starts at its smallest vertex,
 *   2 * min_read, and carries KMU_SG_UNITIG_CIRCULAR; the arc entering the start vertex closes the cycle and is not walked.
 * Coordinates (64 bits): the contribution c(v) is in(v) if v has a unique in-arc -- the start of a cycle has one -- and the length
 *   of its read otherwise.  end of a step (kmu_sg_step: read, strand, end) is the running sum of c along the unitig; len of a
 *   unitig is the end of its last step, so for a cycle the sum of all its arcs' len.
 * Numbering: unitigs are numbered by increasing min_read.  A unitig record (kmu_sg_unitig) is first, len, n_reads, flags, min_read,
 *   0: first is the exclusive prefix sum of n_reads over that numbering, and unitig u's steps are path_out[first .. first +
 *   n_reads).  place_out[r] (kmu_sg_place) = {unitig, rank within it, strand, 0}.  *n_out is the number of unitigs, *n_steps_out
 *   the number of reads placed (both host memory in both modes); records beyond those counts are left untouched.  Both counts are
 *   <= n_reads, so there is no count call.
 * n_arcs == 0: every read that is not contained is its own unitig.  n_reads == 0: KMU_OK with zero unitigs.
 * KMU_E_BAD_ARG (nothing is launched): null ctx / offsets / n_out / unitigs_out / path_out, null arcs with n_arcs > 0, bad mem,
 *   arcs while there are no reads.  KMU_E_UNSUPPORTED: n_reads >= 2^31; the arc faults.
 * KMU_MEM_DEVICE: every array except n_steps_out and n_out is device memory; the call synchronises the stream once, for the two
 *   counts and the refusal flag, also in async_device contexts.  KMU_MEM_HOST: the arrays go up through the context's workspace and
 *   the results come back.
 * How: one lane per arc checks and links; one lane per vertex tests the mate; list ranking by pointer doubling backwards over prev,
 *   ceil(log2(2 n_reads)) launches that read one buffer and write the other; the smallest vertex of every cycle is cut loose and the
 *   rounds are launched once more (they return at once where nothing was cut); tails publish at their head, two scans over the reads number the unitigs and place their steps; one lane
 *   per vertex writes.  The launch count depends on n_reads only.  Integer compares, idempotent stores and commuting integer
 *   atomics only.  DESIGN.md 3.23 has the kernels.
 *
 * kmu_sg_unitig_seqs.  unitigs[n_unitigs] and path[n_steps] as kmu_sg_unitigs writes them (or any records that pass the checks
 *   below; unitigs may share steps), bases and offsets[n_reads + 1] of the batch.  The sequence of a unitig is the concatenation
 *   over its steps of the last c bytes of the read in the step's orientation, c = end - previous end with a previous end of 0 at
 *   the first step.  Strand 0 copies bytes verbatim; strand 1 is the reverse complement: A<->T, C<->G, a<->t, c<->g, every other
 *   byte N.  seq_offsets_out[n_unitigs + 1] (may be NULL) are the unitigs' offsets into seq_out.
 *   *n_out (host memory in both modes) is always the total byte count.  seq_out == NULL: the count-only call, which writes *n_out
 *   and nothing else.  cap < total: KMU_E_BAD_ARG with *n_out set and nothing else written.
 *   KMU_E_BAD_ARG: null ctx / offsets / n_out, unitigs null with n_unitigs > 0, path null with n_steps > 0, bases null while bytes
 *   are to be written, bad mem.  KMU_E_UNSUPPORTED, found on the device BEFORE anything is written (the outputs stay untouched):
 *   first + n_reads > n_steps; a step's read >= n_reads; a strand > 1; ends decrease; a contribution above the read's length; the
 *   last end is not len (a unitig without steps has len 0).  No record is used as an address before the check.
 *   KMU_MEM_DEVICE: every array except n_out is device memory; two synchronisations (the check with the totals; the end).
 *   How: an ITEM is a step of a unitig.  One lane per unitig checks its slice; scans give the offsets and the item numbering; one
 *   lane per item finds its unitig by binary search and checks its step; after the synchronisation one lane per item stores its
 *   global end seq_offsets[u] + end, and one wave per tile of 4096 OUTPUT bytes finds the item of its first byte by a 64-ary search
 *   over those ends and walks on 64 bytes at a time, one per lane, as kmu_extract_ranges does. */
#define KMU_SG_NONE 0xFFFFFFFFu
#define KMU_SG_UNITIG_CIRCULAR 1u  /* kmu_sg_unitig.flags */
typedef struct {         /* 16 bytes: one read of a path */
    uint32_t read, strand;
    uint64_t end;
} kmu_sg_step;
typedef struct {         /* 32 bytes */
    uint64_t first, len;
    uint32_t n_reads, flags, min_read, zero;
} kmu_sg_unitig;
typedef struct {         /* 16 bytes: per read */
    uint32_t unitig, rank, strand, zero;
} kmu_sg_place;
int kmu_sg_unitigs(kmu_ctx *ctx, const kmu_sg_arc *arcs, uint64_t n_arcs,
                   const kmu_sg_read *reads,    /* may be NULL */
                   const uint64_t *offsets, uint32_t n_reads, int mem,
                   kmu_sg_unitig *unitigs_out,  /* room for n_reads */
                   kmu_sg_step *path_out,       /* room for n_reads */
                   kmu_sg_place *place_out,     /* n_reads; may be NULL */
                   uint64_t *n_steps_out,       /* host memory in both modes; may be NULL */
                   uint64_t *n_out);            /* host memory in both modes; required */
int kmu_sg_unitig_seqs(kmu_ctx *ctx, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path,
                       uint64_t n_steps, const uint8_t *bases, const uint64_t *offsets, uint32_t n_reads, int mem,
                       uint64_t *seq_offsets_out,   /* n_unitigs + 1; may be NULL */
                       uint8_t *seq_out,            /* NULL: the count-only call */
                       uint64_t cap, uint64_t *n_out);

/* ---- string graph cleaning: short dead ends (tips) are removed and simple bubbles are popped --------------------------
 * Inputs: arcs[n_arcs], arc records in the (from, to, rec) order kmu_sg_graph writes them -- only non-decreasing `from` is required
 *   (and checked, over EVERY arc: the slices out(v) are found by binary search over the whole list, no offsets are passed);
 *   reads[n_reads], the summaries, or NULL (then no read is contained and the summaries written are otherwise zero).
 * An arc SURVIVES iff flags == 0, so the output of one call is a valid input of the next.  out(v) counts the surviving arcs of v;
 *   in(v) = out(v ^ 1), which by mate symmetry is the number of surviving arcs that enter v.
 * Phase 1, tips; off when max_tip_reads == 0.  T = max_tip_reads.  v0 is a tip start iff in(v0) = 0 and out(v0) = 1.  Walk
 *   v(i+1) = the target of the only surviving arc of v(i).  On arriving at w from v(i) the reads so far are v0 .. v(i): if
 *   in(w) >= 2 the walk ends and is a CANDIDATE tip of i + 1 reads with junction w iff i + 1 <= T; otherwise, if out(w) = 1 and
 *   i + 1 < T, the walk continues with w; otherwise it is no tip (a line that ends, a stem before a fork, or too long).
 *   Spare rule: the in-neighbours of a junction w are to ^ 1 over the surviving arcs of out(w ^ 1).  When ALL of them are last
 *   vertices of candidate tips, the candidate with the most reads is spared, at equal counts the one whose last vertex id is
 *   smallest; n_spared counts such junctions.  (Without it a contig whose end forks into two short ends would lose both.)
 *   Every read of a candidate that is not spared gets KMU_SG_READ_TIP, and every surviving arc that touches such a read, at either
 *   end and on either strand, gets KMU_SG_ARC_TIP.  n_tips and n_tip_reads count the removed candidates and their reads.  A tip
 *   that LEAVES a junction needs no rule: it is the twin of a tip that enters w ^ 1, and the removal is per read.
 * Phase 2, simple bubbles; off when max_bubble_reads == 0.  B = max_bubble_reads.  The degrees are those over the arcs that survive
 *   phase 1.  s is a source iff out(s) = 2.  A branch of s is a1 .. ak with s -> a1 -> ... -> ak -> t, 1 <= k <= B,
 *   in(aj) = out(aj) = 1 for every j, and in(t) = 2 exactly.  A bubble is a source whose two branches both exist and end at the same
 *   t with t >> 1 != s >> 1.  The two interiors are then disjoint as reads.  Proof: from an interior vertex x the walk forwards is
 *   forced, so the first vertex that is not interior reached from x is unique: t; backwards likewise: s.  The twin map sends the
 *   branch through x to the branch through x ^ 1 of the bubble with source t ^ 1 and end s ^ 1.  A read with x on one branch and
 *   x ^ 1 on the other would give x ^ 1 the end t as well as s ^ 1, so t = s ^ 1, which is excluded.
 *   The branch with fewer interior reads loses; at equal counts the branch that does NOT hold the smallest interior read id loses.
 *   The rule is invariant under the twin map, so s and t ^ 1 decide alike.  The loser's interior reads get KMU_SG_READ_BUBBLE, the
 *   surviving arcs that touch them KMU_SG_ARC_BUBBLE.  All bubbles are decided on the same graph, then removed.  n_bubbles counts
 *   each bubble once (at the smaller of s and t ^ 1), n_bubble_reads the removed reads.
 * Finish: arcs_out[i] is arcs[i] with the new flag; `unique` is recomputed for every arc by the rule of kmu_sg_graph over the arcs
 *   with flags == 0, an arc with any flag has unique = 0.  reads_out[r] is reads[r] (zero where reads is NULL) with the new flag
 *   bits OR-ed in and out_fwd, out_rev the final surviving degrees.  n_arcs_tip, n_arcs_bubble: the arcs flagged by this call;
 *   n_arcs_left: the arcs whose flags are still 0.  Removal is per read and the mate of an arc touches the same two reads, so the
 *   result is mate-symmetric and kmu_sg_unitigs accepts it; reads that carry TIP or BUBBLE stay single-read unitigs there unless
 *   the caller also marks them KMU_SG_READ_CONTAINED.
 * KMU_E_BAD_ARG (nothing is launched): null ctx / p / stats_out; null arcs or arcs_out with n_arcs > 0; non-zero flags or zero; a
 *   limit above KMU_SG_CLEAN_MAX; bad mem; arcs while there are no reads; arcs_out overlapping arcs.
 * KMU_E_UNSUPPORTED: n_reads >= 2^31, n_arcs >= 2^32, and the faults, found on the device; the call is refused at its one
 *   synchronisation, every output (stats_out included) is left untouched and no faulty arc is used as an index: `from` decreases
 *   from one arc to the next; in a surviving arc, from or to >= 2 n_reads, or from >> 1 == to >> 1; a surviving arc v -> w with rec
 *   c has no surviving arc w^1 -> v^1 with rec c; with reads, a surviving arc touches a read flagged KMU_SG_READ_CONTAINED.
 * n_arcs == 0: KMU_OK with zero stats; reads_out is the input summaries with zero degrees.  n_reads == 0: KMU_OK, zero stats.
 * KMU_MEM_DEVICE: arcs, reads, arcs_out and reads_out are device memory; one synchronisation, which hands over the stats and the
 *   refusal flag, also in async_device contexts.  KMU_MEM_HOST: the arrays go up through the context's workspace and come back.
 * The result is a pure function of the input: integer compares, idempotent stores and commuting integer atomics only.  "The only
 *   surviving arc of v" is the smallest target over out(v), kept by an atomic minimum, and is read only where out(v) = 1.
 * How: one lane per arc checks, counts the degrees and keeps the sole successor; one lane per vertex walks a tip and publishes its
 *   read count at its last vertex; one lane per junction applies the spare rule; one lane per tip start walks again and flags; one
 *   lane per arc flags and recounts; one lane per source walks both branches and the loser again; one lane per arc flags and
 *   recounts; one lane per arc sets unique; one lane per read writes its summary.  Nine launches whatever the graph; every walk is at
 *   most KMU_SG_CLEAN_MAX dependent loads.  DESIGN.md 3.24 has the kernels. */
#define KMU_SG_ARC_TIP     2u   /* kmu_sg_arc.flags */
#define KMU_SG_ARC_BUBBLE  4u
#define KMU_SG_READ_TIP    2u   /* kmu_sg_read.flags */
#define KMU_SG_READ_BUBBLE 4u
#define KMU_SG_CLEAN_MAX   64u  /* largest max_tip_reads / max_bubble_reads */
typedef struct {
    uint32_t max_tip_reads;     /* 0: no tip removal */
    uint32_t max_bubble_reads;  /* 0: no bubble popping */
    uint32_t flags;             /* no flag bits yet: must be 0 */
    uint32_t zero;
} kmu_sg_clean_params;
typedef struct {
    uint64_t n_tips, n_tip_reads, n_spared, n_bubbles, n_bubble_reads, n_arcs_tip, n_arcs_bubble, n_arcs_left;
} kmu_sg_clean_stats;
int kmu_sg_clean(kmu_ctx *ctx, const kmu_sg_arc *arcs, uint64_t n_arcs,
                 const kmu_sg_read *reads,       /* may be NULL */
                 uint32_t n_reads, const kmu_sg_clean_params *p, int mem,
                 kmu_sg_arc *arcs_out,           /* n_arcs; must not overlap arcs */
                 kmu_sg_read *reads_out,         /* n_reads; may be NULL */
                 kmu_sg_clean_stats *stats_out); /* host memory in both modes; required */

/* ---- unitig map: one chain record per read saying where the read lies on which unitig ---------------------------------
 * The layout already knows where every read lies, so no seeding or chaining against the unitig bases is needed: the records written
 *   here feed kmu_chain_cigar / kmu_chain_pileup / ... with the unitig batch (seq, seq_offsets of kmu_sg_unitig_seqs) as the q side
 *   and the reads as the db side, votes with KMU_PILE_Q, which is the consensus over a unitig's reads.
 * Inputs: unitigs[n_unitigs], path[n_steps] and place[n_reads] as kmu_sg_unitigs writes them; chains[n_chains] and
 *   classes[n_chains], the self-join and the class_out of kmu_sg_graph / kmu_sg_classify (both may be NULL with n_chains == 0: then
 *   no contained read is placed); offsets[n_reads + 1] of the batch -- only the lengths are used.
 * Output: at most one record per read, in ascending read id; out has room for n_reads, there is no count call; *n_out (host memory)
 *   is the number of records.  read_a = the unitig, read_b = the read, strand as kmu_chain_align reads it, score = 0 for a layout
 *   read and 1 for a contained read, n_seeds = the index of the containment record or KMU_SG_NONE, n_anchors = the container read
 *   or KMU_SG_NONE.
 * Layout read: place[r] = {u, rank, s}, its step path[unitigs[u].first + rank] has end e, the read has length L, t = min(L, e):
 *   a = [e - t, e), b = the last t bases of the read in the step's orientation, [L - t, L) for s = 0 and [0, t) for s = 1;
 *   strand = s.  t < L at the start of a circular unitig and wherever a later read is longer than everything before it.
 * Contained read: place[c].unitig == KMU_SG_NONE.  Chain x is a CANDIDATE iff classes[x] == KMU_SG_A_CONTAINED and read_a == c
 *   (the container is g = read_b, c's segment [cs, ce) is the a segment, g's segment [gs, ge) the b segment) or classes[x] ==
 *   KMU_SG_B_CONTAINED and read_b == c (g = read_a, the segments the other way round) -- no other class is looked at --, g is
 *   placed (one level only: a read contained only in contained reads stays unplaced), and, with g's step (sg, e_g), its length L_g
 *   and os = gs for sg = 0, L_g - ge for sg = 1, a_start = e_g - L_g + os (signed 64 bits) is >= 0.  The winner is the candidate
 *   with the largest ce - cs, at equal lengths the smallest x: one 64-bit atomic maximum of (ce - cs) << 32 | (2^32 - 1 - x) per
 *   contained read, so timing changes nothing.  Its record: a = [a_start, a_start + (ge - gs)) on g's unitig, b = [cs, ce),
 *   strand = sg ^ the record's strand.
 * The a coordinates are NOMINAL: the last c bytes of a read sit exactly where its record says; its earlier bytes lie on stretches
 *   copied from other reads, so the record is off there by the indel drift between the reads, which the band of the alignment
 *   absorbs.  On error-free reads the coordinates are exact (overlap hangs are differences on one diagonal).
 * stats_out (host memory): n_layout reads with a place, n_contained contained reads with a winner, n_unplaced the rest.
 * KMU_E_BAD_ARG (nothing is launched): null ctx / p / offsets / out / stats_out / n_out; unitigs, path or place null while their
 *   count is > 0 (place: n_reads); chains or classes null with n_chains > 0; non-zero flags or zero; bad mem.
 * KMU_E_UNSUPPORTED: n_chains >= 2^32, n_reads >= 2^31, and the faults, found on the device; the call is refused at its one
 *   synchronisation, every output (stats_out and n_out included) is left untouched and no faulty record is used as an index:
 *   a unitig with first + n_reads > n_steps or len >= 2^32 (kmu_chain holds 32-bit positions); a step with read >= n_reads,
 *   strand > 1 or end == 0; a place with a unitig >= n_unitigs that is not KMU_SG_NONE, a rank >= that unitig's n_reads, a step
 *   that does not name the read with the place's strand, or a step whose end is above the unitig's len; a record of class
 *   A_CONTAINED or B_CONTAINED with a read >= n_reads, strand > 1, a start above its end or an end above its read's length.
 * n_reads == 0: KMU_OK with zero counts.
 * KMU_MEM_DEVICE: every array except p, stats_out and n_out is device memory; one synchronisation, which hands over the counts and
 *   the refusal flag, also in async_device contexts.  KMU_MEM_HOST: the arrays go up through the context's workspace and the
 *   records come back.
 * How: one lane per unitig / step / place checks; one lane per chain tests candidacy and does the atomic maximum; one lane per read
 *   decides whether it has a record; a scan over the reads; one lane per read writes.  Four kernels and a scan whatever the data;
 *   integer compares, idempotent stores and commuting integer atomics only.  DESIGN.md 3.25 has the kernels. */
typedef struct {
    uint32_t flags;             /* no flag bits yet: must be 0 */
    uint32_t zero;
} kmu_um_params;
typedef struct {
    uint64_t n_layout, n_contained, n_unplaced;
} kmu_um_stats;
int kmu_sg_unitig_chains(kmu_ctx *ctx, const kmu_sg_unitig *unitigs, uint64_t n_unitigs, const kmu_sg_step *path,
                         uint64_t n_steps,
                         const kmu_sg_place *place,   /* n_reads, as kmu_sg_unitigs wrote it */
                         const kmu_chain *chains, const uint8_t *classes, uint64_t n_chains, /* may be NULL with n_chains == 0 */
                         const uint64_t *offsets, uint32_t n_reads, const kmu_um_params *p, int mem,
                         kmu_chain *out,              /* room for n_reads */
                         kmu_um_stats *stats_out,     /* host memory in both modes; required */
                         uint64_t *n_out);            /* host memory in both modes; required */

#ifdef __cplusplus
}
#endif
#endif /* KMU_H */
